"""gpu: the context-level operators of csrc/ops.hip share ONE workspace (gr_ctx.ws), which each call carves into regions.  The suites of
the single calls cover their arithmetic; this file covers what the shared staging can break: a region that overlaps its neighbour or is
misaligned at odd sizes, and a pointer taken before the workspace grew."""
import numpy as np
import pytest

import imagegrid_oracle as io_
import progress_oracle as po

pytestmark = pytest.mark.gpu
F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return (a.dtype.str, a.shape, a.tobytes())


def same(got, want, what):
    """bit for bit, element type and shape included"""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert bits(g) == bits(w), f"{what}[{i}]"


def run_every_wrapper(c, oracle, n, d, k):
    """Every wrapper that stages through the workspace, once, at n rows of d floats / n images of 3 x 5 x 7, in the context c.  Each host
    call is compared with its device twin on buffers of c.malloc (or, where there is none, with the numpy / oracle twin the call's own
    suite uses) -> {call: [arrays]} for the comparison between passes."""
    import ganrev._lib as L
    from ganrev import synth
    held, out = [], {}
    up = lambda a: held.append(c.upload(a)) or held[-1]
    room = lambda nbytes: held.append(c.malloc(nbytes)) or held[-1]
    try:
        x, t = synth.uniform((n, d), 11, 0.05, 0.95), synth.uniform((n, d), 12, 0, 1)
        dx, dt, dg, dl = up(x), up(t), room(x.nbytes), room(64)
        for name, host, dev in (("mse", c.mse, c.mse_dev), ("bce", c.bce, c.bce_dev)):
            loss, grad = host(x, t)
            dev(dx, dt, x.size, dl, dg)
            out[name] = [np.array([loss]), grad]
            same(out[name], [np.array([c.read_loss(dl)]), c.download(dg, x.shape)], name)
            same([np.array([host(x, t, want_grad=False)[0]])], out[name][:1], name + " without a gradient")

        img = synth.uniform((n, 3, 5, 7), 13, 0, 1)
        dimg = up(img)
        for to, planes in ((L.GR_CS_YUV, 3), (L.GR_CS_Y, 1)):
            dout = room(4 * n * planes * 35)
            c.colorspace_dev(dimg, 0, to, n, 5, 7, dout)
            out[f"colorspace{to}"] = [c.colorspace(img, 0, to)]
            same(out[f"colorspace{to}"], [c.download(dout, (n, planes, 5, 7))], f"colorspace to {to}")
        dsc = room(4 * n * 3 * 9 * 4)
        c.image_scale_dev(dimg, n, 3, 5, 7, 9, 4, dsc)
        out["image_scale"] = [c.image_scale(img, 9, 4)]
        same(out["image_scale"], [c.download(dsc, (n, 3, 9, 4))], "image_scale")

        v = synth.normal((n, d), 14)
        v[: n // 3] += 1.5
        c0 = v[:k].copy()                                                 # distinct rows: no cluster starts empty
        cent, tot, lab = c.kmeans(v, k, 3, c0)
        rcent, rtot, rlab = oracle.kmeans(v, k, 3, c0)
        assert np.array_equal(lab, rlab) and np.array_equal(tot, rtot) and float(np.abs(cent - rcent).max()) <= 1e-6    # test_gpu_parity's bar
        out["kmeans"] = [cent, tot, lab]
        for take_min in (True, False):
            out[f"cosine_assign{int(take_min)}"] = list(c.cosine_assign(v, rcent, take_min))
            same(out[f"cosine_assign{int(take_min)}"], list(oracle.cosine_assign(v, rcent, take_min)), "cosine_assign")

        w = synth.normal((n, d), 15)
        dv, dw = up(v), up(w)
        out["l2_distance_rows"] = [c.l2_distance_rows(v, w)]
        same(out["l2_distance_rows"], [c.l2_distance_rows_dev(dv, dw, n, d)], "l2_distance_rows")
        out["l2_nearest"] = list(c.l2_nearest(v, w[:2], k))
        same(out["l2_nearest"], list(c.l2_nearest(None, w[:2], k, table_dev=dv, n=n, d=d)), "l2_nearest")
        out["cosine_topk"] = list(c.cosine_topk(v, [0, n - 1], k))
        same(out["cosine_topk"], list(c.cosine_topk(None, [0, n - 1], k, emb_dev=dv, n=n, d=d)), "cosine_topk")

        rows = np.arange(n, dtype=np.int64)[::-1].copy()
        dmean = room(4 * 3 * 35)
        c.rows_mean_dev(dimg, n, 3 * 35, rows, dmean)
        out["rows_mean"] = [c.download(dmean, (3, 5, 7))]
        same(out["rows_mean"], [io_.rows_mean(img, rows)], "rows_mean")
        nrow = max(2, int(np.sqrt(n)))
        cout, (gh, gw) = 3, io_.geometry(n, 1, 5, 7, nrow, 1, 0)[4:6]
        dgrid, du8 = room(4 * cout * gh * gw), room(cout * gh * gw)
        assert c.image_grid_dev([dimg], [n], 3, 5, 7, -1, rows, nrow, padding=1, auto_range=True, grid_dev=dgrid, u8_dev=du8) == (cout, gh, gw)
        out["image_grid"] = [c.download(dgrid, (cout, gh, gw)), c.download(du8, (gh, gw, cout), np.uint8)]
        want = io_.image_grid([img], rows.reshape(-1, 1), nrow, -1, padding=1, auto_range=True)
        same(out["image_grid"], [want, io_.quantise(want)], "image_grid")
        grid_w = nrow
        grid_h = (n + grid_w - 1) // grid_w
        cout, gh, gw = po.shape(3, 5, 7, -1, grid_h, grid_w)
        dgrid, du8 = room(4 * cout * gh * gw), room(cout * gh * gw)
        assert c.progress_grid_dev(dimg, n, 3, 5, 7, -1, rows, grid_h, grid_w, 17, dgrid, du8) == (cout, gh, gw)
        out["progress_grid"] = [c.download(dgrid, (cout, gh, gw)), c.download(du8, (gh, gw, cout), np.uint8)]
        want = po.progress_grid(img, rows, n, grid_h, grid_w, 17)
        same(out["progress_grid"], [want, po.quantise(want)], "progress_grid")
    finally:
        for p in held:
            c.free(p)
    return out


def test_wrappers_share_one_workspace_at_odd_sizes_and_across_its_growth(oracle):
    """One fresh context (its workspace starts empty), three passes without a reset: 7 rows of 5 floats and 3 x 5 x 7 images scaled to
    3 x 9 x 4 (no size a multiple of 4 elements, so a region that is not padded to its boundary starts misaligned); 4099 rows of 33
    floats, which no longer fit the first pass's workspace, so it is freed and allocated again; then the small sizes again, which must
    give the first pass's bits."""
    import ganrev._lib as L
    c = L.Context(0)
    try:
        c.set_conv_mode("f16x3")
        first = run_every_wrapper(c, oracle, 7, 5, 3)
        run_every_wrapper(c, oracle, 4099, 33, 3)
        again = run_every_wrapper(c, oracle, 7, 5, 3)
        assert sorted(first) == sorted(again)
        for name in first:
            same(again[name], first[name], name + " after the workspace grew")
    finally:
        c.close()

