"""gpu: gr_tsne_*_dev and gr_map_cells_dev (csrc/tsne.hip) against float64 numpy (tests/tsne_oracle.py) within the bounds tests/tsne_paths.py
derives from the library's operation chains - every check asserts max err / bound <= 1 and prints the ratio - the update and the cells against
their numpy restatements bit for bit, gr_tsne_run_dev against the public calls it stands for, and ganrev.apply_r --map.  A run of apply_r
without the option makes the calls it made before: here the files of a run with --map are compared with those of the same run without it."""
import contextlib
import json
import os

import numpy as np
import pytest

import tsne_oracle as to
import tsne_paths as tp

pytestmark = pytest.mark.gpu
SIZES = [4, 63, 64, 65, 257, 513, 1025]


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(err).all() and np.isfinite(bound).all()
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def perplexity_for(n):
    return min(30.0, (n - 1) / 3)


def affinities_dev(ctx, x, perplexity):
    """-> (P f32 [n, n], beta f64 [n], info); the outputs start from garbage"""
    n, d = x.shape
    with on_device(ctx, x, np.full((n, n), 7, np.float32), np.full(n, 7.0), np.full(2, 7, np.int32)) as (dx, dp, db, di):
        ctx.tsne_affinities_dev(dx, n, d, perplexity, dp, db, di)
        return ctx.download(dp, (n, n)), ctx.download(db, (n,), np.float64), ctx.download(di, (2,), np.int32)


# ------------------------------------------------------------------ 1. affinities
def check_affinities(ctx, x, perplexity, name):
    n, d = x.shape
    P, beta, info = affinities_dev(ctx, x, perplexity)
    assert np.array_equal(bits(P), bits(P.T.copy()))                                    # symmetric bit for bit
    assert not np.diag(P).any() and np.isfinite(P).all() and (P >= 0).all()
    assert info[1] == 0 and 0 <= info[0] < to.MAX_TRIES                                 # no row at the cap
    r_sum = abs(P.sum(dtype=np.float64) - 1) / tp.total_bound(n)
    D = to.distances(x)
    r_h = max(abs(to.row_entropy(D, i, beta[i]) - np.log(perplexity)) / (to.TOL + tp.entropy_eval_bound(D, d, i, beta[i])) for i in range(n))
    ref, betas, tries = to.joint_from_distances(D, perplexity)
    r_p = worst(np.abs(P - ref), tp.joint_bound(D, d, betas, ref))
    print(f"{name}: n {n} d {d} perplexity {perplexity:g}: updates {info[0]} (numpy {tries.max()}); sum err / bound {r_sum:.3g}, H {r_h:.3g}, P {r_p:.3g}")
    assert r_sum <= 1 and r_h <= 1 and r_p <= 1
    return P, ref, D, betas


@pytest.mark.parametrize("d", [1, 3, 32, 100])
@pytest.mark.parametrize("n", SIZES)
def test_affinities(ctx, n, d):
    check_affinities(ctx, to.gaussian(n, d), perplexity_for(n), "gaussian")


def test_affinities_in_pixel_space(ctx):
    check_affinities(ctx, to.gaussian(65, 3072), 20.0, "pixel space")


def test_affinities_with_duplicate_rows(ctx):
    P, _, _, _ = check_affinities(ctx, to.with_duplicates(65, 8), 10.0, "duplicates")
    assert P[0, 1] > 0 and P[0, 1] == P[0, 32] and np.array_equal(P[0, 2:32], P[1, 2:32])      # rows 0, 1 and 32 are one point


def test_affinities_far_from_the_origin(ctx):
    x = to.far_from_origin(65, 8)
    P, ref, D, betas = check_affinities(ctx, x, 20.0, "mean 1000, sd 1")
    miss = worst(np.abs(to.joint_from_distances(to.one_pass_distances_f32(x), 20.0)[0] - ref), tp.joint_bound(D, 8, betas, ref))
    print(f"the float32 |x|^2 + |y|^2 - 2xy distances: P err / bound {miss:.3g}")
    assert miss > 100                                                                   # the case bites: a one-pass kernel fails it by orders of magnitude


def test_affinities_twice_give_the_same_bits(ctx):
    x = to.gaussian(513, 32)
    a, b = affinities_dev(ctx, x, 30.0), affinities_dev(ctx, x, 30.0)
    for u, v in zip(a, b):
        assert np.array_equal(bits(u), bits(v))


# ------------------------------------------------------------------ 2. gradient and KL
@pytest.mark.parametrize("n", SIZES + [2049])
def test_gradient_and_kl(ctx, n):
    P = to.random_joint(n)
    with on_device(ctx, P, np.zeros((n, 2), np.float32), np.full((n, 2), 7, np.float32), np.full(1, 7.0), np.full(1, 7.0)) as (dp, dy, dg, dz, dk):
        for scale in (1e-4, 1.0, 50.0):
            y = to.layout(n, scale)
            ctx.upload(y, dy)
            ctx.tsne_kl_dev(dp, dy, n, dk)
            kl = float(ctx.download(dk, (1,), np.float64)[0])
            r_kl = abs(kl - to.kl(P, y)) / tp.kl_bound(P, y)
            for e in (1.0, 12.0):
                ctx.tsne_gradient_dev(dp, dy, n, e, dg, dz)
                g, z = ctx.download(dg, (n, 2)), float(ctx.download(dz, (1,), np.float64)[0])
                ref, zref = to.gradient(P, y, e)
                r_g, r_z = worst(np.abs(g - ref), tp.gradient_bound(P, y, e)), abs(z - zref) / (tp.EW * (1 + tp.gamma(n * n)) * zref + tp.gamma(n * n) * zref)
                print(f"n {n} scale {scale:g} e {e:g}: gradient err / bound {r_g:.3g}, Z {r_z:.3g}, KL {r_kl:.3g}")
                assert r_g <= 1 and r_z <= 1 and r_kl <= 1
                ctx.tsne_gradient_dev(dp, dy, n, e, dg, None)                            # z_dev is optional, and a second call gives the same bits
                assert np.array_equal(bits(ctx.download(dg, (n, 2))), bits(g))


# ------------------------------------------------------------------ 3. update
def update_case(n, seed):
    rng = np.random.default_rng([n, seed, 5])
    y, g, inc = (rng.standard_normal((n, 2)).astype(np.float32) for _ in range(3))
    gains = rng.choice(np.float32([0.01, 0.0124, 0.0126, 1.0, 3.2]), (n, 2)).astype(np.float32)      # at the floor, and dropping below it
    for a in (g, inc):                                                                  # +-0 on either side, alone and together
        a[rng.random((n, 2)) < 0.15] = 0.0
        a[rng.random((n, 2)) < 0.15] = -0.0
    return y, g, inc, gains


@pytest.mark.parametrize("n", [5, 512, 513, 1100])
def test_update_has_the_restated_bits(ctx, n):
    y, g, inc, gains = update_case(n, 0)
    want = tp.update(y, g, inc, gains, 50.0, 0.8, 0.01)
    with on_device(ctx, y, g, inc, gains) as (dy, dg, di, dga):
        ctx.tsne_update_dev(dy, dg, di, dga, n, 50.0, 0.8, 0.01)
        got = [ctx.download(p, (n, 2)) for p in (dy, di, dga)]
        assert np.array_equal(bits(ctx.download(dg, (n, 2))), bits(g))                   # the gradient is read only
    for name, a, b in zip(("y", "inc", "gains"), got, want):
        assert np.array_equal(bits(a), bits(b)), name
    assert got[2].min() == np.float32(0.01)
    r = worst(np.abs(got[0].astype(np.float64).mean(axis=0)), tp.mean_bound(want[3], want[0]))
    print(f"n {n}: column means of the result / bound {r:.3g}")
    assert r <= 1


# ------------------------------------------------------------------ 4. the run
def run_state(ctx, n):
    return on_device(ctx, to.layout(n, 1e-4, 3), np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32), np.full(8, 7.0))


def test_run_is_the_sequence_of_public_calls(ctx):
    import ganrev._lib as L
    n, iters, every = 300, 40, 7
    x, _ = to.blobs(n, 32, 5)
    cfg = L.TsneConfig(eta=50.0, exaggeration=12.0, stop_lying_iter=10, mom_switch_iter=20)
    with on_device(ctx, x, np.zeros((n, n), np.float32), np.zeros(2, np.int32), np.zeros((n, 2), np.float32)) as (dx, dp, dinfo, dg):
        ctx.tsne_affinities_dev(dx, n, 32, 30.0, dp, None, dinfo)                        # beta_dev is optional

        def state(y, inc, gains, kl):
            return [ctx.download(p, (n, 2)) for p in (y, inc, gains)] + [ctx.download(kl, (8,), np.float64)]
        with run_state(ctx, n) as (y, inc, gains, kl):
            ctx.tsne_run_dev(dp, n, cfg, y, inc, gains, 0, iters, kl, every)
            whole = state(y, inc, gains, kl)
        with run_state(ctx, n) as (y, inc, gains, kl):                                   # the same from Python, one public call after the other
            for t in range(iters):
                e, mom = tp.schedule(t, 12.0, 10, 20)
                ctx.tsne_gradient_dev(dp, y, n, e, dg)
                ctx.tsne_update_dev(y, dg, inc, gains, n, 50.0, mom, 0.01)
                if (t + 1) % every == 0:
                    ctx.tsne_kl_dev(dp, y, n, kl + 8 * ((t + 1) // every - 1))
            public = state(y, inc, gains, kl)
        with run_state(ctx, n) as (y, inc, gains, kl):                                   # split in two calls
            ctx.tsne_run_dev(dp, n, cfg, y, inc, gains, 0, 17, kl, every)
            ctx.tsne_run_dev(dp, n, cfg, y, inc, gains, 17, 23, kl, every)
            split = state(y, inc, gains, kl)
        with run_state(ctx, n) as (y, inc, gains, kl):                                   # a second run
            ctx.tsne_run_dev(dp, n, cfg, y, inc, gains, 0, iters, kl, every)
            again = state(y, inc, gains, kl)
        with run_state(ctx, n) as (y, inc, gains, kl):                                   # no KL asked for: none written, the same map
            ctx.tsne_run_dev(dp, n, cfg, y, inc, gains, 0, iters, None, every)
            ctx.tsne_run_dev(dp, n, cfg, y, inc, gains, iters, 0, kl, 0)
            silent = state(y, inc, gains, kl)
    assert np.isfinite(whole[0]).all() and np.abs(whole[0]).max() > 1e-3                 # the map has moved
    assert (whole[3][:5] != 7.0).all() and (whole[3][5:] == 7.0).all() and (silent[3] == 7.0).all()      # 40 // 7 values
    for name, other in (("public calls", public), ("17 + 23", split), ("second run", again)):
        for a, b in zip(whole, other):
            assert np.array_equal(bits(a), bits(b)), name
    for a, b in zip(whole[:3], silent[:3]):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("n,d,c,perplexity", [(64, 3, 4, 10), (300, 32, 5, 30), (600, 32, 6, 30)])
def test_blobs_stay_together_in_the_map(ctx, n, d, c, perplexity, seed):
    """Measured on the MI355X (DESIGN.md has the table): purity 1.0 on every case; the final KL next to the float64 twin's is printed, not
    asserted - the dynamics amplify rounding, so two correct runs differ."""
    from ganrev import tsne as T
    x, labels = to.blobs(n, d, c, seed)
    with on_device(ctx, x) as (dx,):
        e = T.embed(ctx, dx, n, d, perplexity=perplexity)
        try:
            P, y, kl, its = e.matrix(), e.y, e.kl, e.kl_iterations
            y0 = T.initialLayout(ctx, dx, n, d)
            assert e.capped == 0 and e.eta == 50.0 and its == list(range(0, 1001, 50)) and np.array_equal(bits(ctx.download(e.y_dev, (n, 2))), bits(y))
        finally:
            e.close()
    twin = to.run(P, y0, 1000, 50.0)
    p1, p10 = to.purity(y, labels, 1), to.purity(y, labels, 10)
    r_kl = abs(kl[-1] - to.kl(P, y)) / tp.kl_bound(P, y)
    print(f"n {n} d {d} c {c} seed {seed}: purity {p1:g} / {p10:g} (float64 twin {to.purity(twin, labels, 1):g} / {to.purity(twin, labels, 10):g}); "
          f"KL {kl[0]:.4f} -> {kl[-1]:.4f} (twin {to.kl(P, twin):.4f}); reported KL err / bound {r_kl:.3g}")
    assert np.isfinite(y).all() and np.isfinite(kl).all()
    assert p1 == 1.0 and p10 == 1.0
    assert r_kl <= 1 and kl[-1] < kl[0]
    assert abs(kl[0] - to.kl(P, y0)) <= tp.kl_bound(P, y0)


def test_random_start(ctx):
    from ganrev import tsne as T
    x, labels = to.blobs(300, 32, 5)
    with on_device(ctx, x) as (dx,):
        a, b, c = (T.initialLayout(ctx, dx, 300, 32, "random", seed) for seed in (1, 1, 2))
        assert np.array_equal(a, b) and not np.array_equal(a, c) and abs(a[:, 0].astype(np.float64).std() - T.INIT_SD) < 1e-9
        e = T.embed(ctx, dx, 300, 32, init="random", seed=3, iterations=500, kl_every=0)
        try:
            assert e.kl_iterations == [0, 500] and e.kl[1] < e.kl[0] and to.purity(e.y, labels, 1) == 1.0
        finally:
            e.close()
        with pytest.raises(Exception, match="init"):
            T.embed(ctx, dx, 300, 32, init="spectral")


# ------------------------------------------------------------------ 6. cells
def cells_dev(ctx, y, gh, gw, counts=True):
    from ganrev import tsne as T
    with on_device(ctx, y) as (dy,):
        return T.mapCells(ctx, dy, len(y), gh, gw, counts=counts)


CELL_CASES = {
    "borders_and_edge": np.float32([[0, 0], [4, 4], [1, 1], [3, 1], [2, 2], [1, 3], [0.9, 0.9]]),
    "degenerate_axis": np.float32([[5, 1], [5, 2], [5, 3]]),
    "one_point": np.float32([[2, 3]]),
    "ties": np.float32([[0, 0], [8, 8], [3, 3], [5, 5], [5, 3], [3, 5], [1, 1], [7, 7]]),
    "random": to.layout(1000, 20.0),
    "two_blocks": to.layout(5000, 1.0, 1),
}


@pytest.mark.parametrize("g", [1, 2, 32])
@pytest.mark.parametrize("name", sorted(CELL_CASES))
def test_cells_have_the_restated_rows(ctx, name, g):
    y = CELL_CASES[name]
    rows, counts = cells_dev(ctx, y, g, g)
    want_rows, want_counts = tp.cells(y, g, g)
    assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts)
    assert counts.sum() == len(y) and ((rows >= 0) == (counts > 0)).all()
    if g == 32:
        assert len(y) >= 1024 or (rows == -1).any()                                     # fewer rows than cells: empty ones


def test_cells_of_a_rectangular_grid_and_without_counts(ctx):
    y = CELL_CASES["random"]
    rows = cells_dev(ctx, y, 3, 7, counts=False)
    assert rows.shape == (3, 7) and np.array_equal(rows, tp.cells(y, 3, 7)[0])           # axis 0 runs along grid_w


# ------------------------------------------------------------------ 7. contracts
def test_limits(ctx):
    import ganrev._lib as L
    n, d = 8, 3
    x = to.gaussian(n, d)
    cfg = L.TsneConfig(eta=50.0)
    hosts = (x, np.full((n, n), 7, np.float32), np.full(n, 7.0), np.full(2, 7, np.int32), np.full((n, 2), 7, np.float32), np.full((n, 2), 7, np.float32),
             np.full((n, 2), 7, np.float32), np.full((n, 2), 7, np.float32), np.full(4, 7.0), np.full(4, 7, np.int64), np.full(4, 7, np.int32))
    with on_device(ctx, *hosts) as ptrs:
        dx, dp, db, di, dy, dg, dinc, dgains, dk, drows, dcounts = ptrs
        refused = [
            (lambda: ctx.tsne_affinities_dev(dx, 3, d, 1.0, dp, db, di), "GR_ERR_INVALID", "n 3"),
            (lambda: ctx.tsne_affinities_dev(dx, n, 0, 2.0, dp, db, di), "GR_ERR_INVALID", "d 0"),
            (lambda: ctx.tsne_affinities_dev(dx, n, d, 0.5, dp, db, di), "GR_ERR_INVALID", "perplexity 0.5"),
            (lambda: ctx.tsne_affinities_dev(dx, n, d, 2.5, dp, db, di), "GR_ERR_INVALID", "perplexity 2.5"),
            (lambda: ctx.tsne_affinities_dev(dx, n, d, float("nan"), dp, db, di), "GR_ERR_INVALID", "perplexity"),
            (lambda: ctx.tsne_affinities_dev(dx, 16385, d, 30.0, dp, db, di), "GR_ERR_UNSUPPORTED", "n 16385: at most GR_TSNE_MAX_N = 16384"),
            (lambda: ctx.tsne_affinities_dev(None, n, d, 2.0, dp, db, di), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_affinities_dev(dx, n, d, 2.0, None, db, di), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_affinities_dev(dx, n, d, 2.0, dp, db, None), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_gradient_dev(dp, dy, 0, 1.0, dg), "GR_ERR_INVALID", "n 0"),
            (lambda: ctx.tsne_gradient_dev(dp, dy, 16385, 1.0, dg), "GR_ERR_UNSUPPORTED", "n 16385"),
            (lambda: ctx.tsne_gradient_dev(None, dy, n, 1.0, dg), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_gradient_dev(dp, None, n, 1.0, dg), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_gradient_dev(dp, dy, n, 1.0, None), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_update_dev(dy, dg, dinc, dgains, 0, 50.0, 0.5), "GR_ERR_INVALID", "n 0"),
            (lambda: ctx.tsne_update_dev(dy, dg, dinc, dgains, 16385, 50.0, 0.5), "GR_ERR_UNSUPPORTED", "n 16385"),
            (lambda: ctx.tsne_update_dev(None, dg, dinc, dgains, n, 50.0, 0.5), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_update_dev(dy, None, dinc, dgains, n, 50.0, 0.5), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_update_dev(dy, dg, None, dgains, n, 50.0, 0.5), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_update_dev(dy, dg, dinc, None, n, 50.0, 0.5), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_kl_dev(dp, dy, 0, dk), "GR_ERR_INVALID", "n 0"),
            (lambda: ctx.tsne_kl_dev(dp, dy, 16385, dk), "GR_ERR_UNSUPPORTED", "n 16385"),
            (lambda: ctx.tsne_kl_dev(dp, dy, n, None), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_run_dev(dp, 16385, cfg, dy, dinc, dgains, 0, 1), "GR_ERR_UNSUPPORTED", "n 16385"),
            (lambda: ctx.tsne_run_dev(dp, n, None, dy, dinc, dgains, 0, 1), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_run_dev(dp, n, cfg, None, dinc, dgains, 0, 1), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.tsne_run_dev(dp, n, cfg, dy, dinc, dgains, -1, 1), "GR_ERR_INVALID", "first_iter -1"),
            (lambda: ctx.tsne_run_dev(dp, n, cfg, dy, dinc, dgains, 0, -1), "GR_ERR_INVALID", "iters -1"),
            (lambda: ctx.tsne_run_dev(dp, n, cfg, dy, dinc, dgains, 0, 1, dk, -1), "GR_ERR_INVALID", "kl_every -1"),
            (lambda: ctx.map_cells_dev(dy, 0, 2, 2, drows, dcounts), "GR_ERR_INVALID", "n 0"),
            (lambda: ctx.map_cells_dev(dy, n, 0, 2, drows, dcounts), "GR_ERR_INVALID", "grid 0 x 2"),
            (lambda: ctx.map_cells_dev(dy, n, 2, 1025, drows, dcounts), "GR_ERR_UNSUPPORTED", "grid 2 x 1025"),
            (lambda: ctx.map_cells_dev(dy, 1 << 31, 2, 2, drows, dcounts), "GR_ERR_UNSUPPORTED", "n 2147483648"),
            (lambda: ctx.map_cells_dev(None, n, 2, 2, drows, dcounts), "GR_ERR_INVALID", "null pointer"),
            (lambda: ctx.map_cells_dev(dy, n, 2, 2, None, dcounts), "GR_ERR_INVALID", "null pointer"),
        ]
        for call, code, word in refused:
            with pytest.raises(L.GanrevError, match=code) as e:
                call()
            assert word in str(e.value), str(e.value)
        ctx.synchronize()
        for p, h in zip(ptrs, hosts):                                                   # nothing was launched: every buffer is as it was
            assert np.array_equal(bits(ctx.download(p, h.shape, h.dtype)), bits(h))
    from ganrev import tsne as T
    with pytest.raises(L.GanrevError, match="GR_TSNE_MAX_N = 16384"):
        T.affinities(ctx, 0, 16385, 3, 30)
    with pytest.raises(L.GanrevError, match="perplexity"):
        T.embed(ctx, 0, 64, 3, perplexity=30)
    P, _, _ = affinities_dev(ctx, x, 2.0)                                               # the context stays usable
    assert abs(P.sum(dtype=np.float64) - 1) <= tp.total_bound(n)


# ------------------------------------------------------------------ 8. the script
BASE = ["--synthetic", "3x32x32x32", "--nbImages", "520", "--quiet", "--render", "--resident"]
MAP_FILES = ("map_y.npy", "map_kl.npy", "map_cells.npy", "map.png")


def run_apply_r(tmp, name, *options):
    from ganrev import apply_r
    where = tmp / name
    summary = apply_r.main(BASE + list(options) + ["--writeTo", str(where)])
    return where, summary


@pytest.fixture(scope="module")
def map_run(tmp_path_factory):
    """a --map run, with what it handed to render.map_grid and the same grid drawn by gr_image_grid_dev while the image table was there"""
    from ganrev import render
    seen, original = {}, render.map_grid

    def spy(images_dev, cell_rows, from_space="rgb", labels=None, path=None):
        seen.update(cells=np.array(cell_rows), labels=None if labels is None else np.array(labels), space=from_space)
        seen["direct"] = render.grid(images_dev, np.asarray(cell_rows).reshape(-1), cell_rows.shape[1], from_space, margin=1, bg=render.map_colours(cell_rows, labels))
        return original(images_dev, cell_rows, from_space, labels, path)
    render.map_grid = spy
    try:
        where, summary = run_apply_r(tmp_path_factory.mktemp("map"), "mapped", "--map", "--mapIterations", "300")
    finally:
        render.map_grid = original
    return where, summary, seen


def test_apply_r_map_writes_its_products(ctx, map_run):
    import ganrev._lib as L
    from ganrev import png, render
    where, summary, seen = map_run
    y, kl, cells = (np.load(where / f) for f in MAP_FILES[:3])
    assert (y.shape, y.dtype, cells.shape, cells.dtype) == ((520, 2), np.float32, (32, 32), np.int64)
    assert kl.shape == (7, 2) and kl[:, 0].tolist() == [0, 50, 100, 150, 200, 250, 300] and np.isfinite(kl).all() and kl[-1, 1] < kl[0, 1]
    entry = json.load(open(where / "summary.json"))["map"]
    assert entry == summary["map"] and entry["rows"] == 520 and entry["d"] == 32 and entry["grid"] == 32 and entry["iterations"] == 300
    assert entry["perplexity"] == 30.0 and entry["eta"] == 50.0 and entry["beta_capped_rows"] == 0 and entry["space"] == "attributes"
    assert entry["kl_first"] == kl[0, 1] and entry["kl_last"] == kl[-1, 1] and entry["cells_filled"] == int((cells >= 0).sum())
    assert np.isfinite(y).all() and np.array_equal(cells, tp.cells(y, 32, 32)[0])        # the cells of the map that was written
    shown = cells[cells >= 0]
    assert 0 < len(shown) <= 520 and len(set(shown.tolist())) == len(shown)
    # the picture: gr_image_grid_dev over map_cells.npy, one tile per cell, -1 left as background, a 1-pixel ring per tile
    picture = png.read_png(str(where / "map.png"))
    assert np.array_equal(seen["cells"], cells) and np.array_equal(picture, seen["direct"])
    _, gh, gw = L.grid_shape(32 * 32, 1, 3, 32, 32, 0, 32, 0, 1)
    assert picture.shape == (gh, gw, 3) == (32 * 34, 32 * 34, 3)
    tiles = picture.reshape(32, 34, 32, 34, 3).transpose(0, 2, 1, 3, 4)                 # [cell row][cell column][34][34][3]
    empty = tiles[cells < 0]
    assert len(empty) and not empty.any()                                               # an empty cell stays MAP_FIELD, ring and all
    # the rings: the colour of the row's cluster - the rows the clustering step kept for a cluster carry that cluster's colour
    labels = seen["labels"]
    assert labels is not None and (labels[shown] >= 0).all() and (np.delete(labels, shown) == -1).all()
    clusters = np.load(where / "cluster_centroids.npy")
    assert len(clusters) == 20 and labels.max() < 20
    ring = tiles[cells >= 0][:, 0, 0, :]                                                # the top-left pixel of every shown tile
    want = np.minimum(255, np.trunc(np.float32(render.MAP_PALETTE)[labels[shown] % 12] * 255 + 0.5)).astype(np.uint8)
    assert np.array_equal(ring, want)


def test_apply_r_without_map_writes_the_same_files(map_run, tmp_path):
    where, summary, _ = map_run
    plain, psummary = run_apply_r(tmp_path, "plain")
    names = sorted(os.listdir(plain))
    assert "map" not in psummary and not [f for f in names if f.startswith("map")]
    assert sorted(os.listdir(where)) == sorted(names + list(MAP_FILES))
    for f in names:
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(where / f, "rb").read(), f
    timing = "embed_and_search_seconds"
    assert {k: v for k, v in summary.items() if k not in ("map", timing)} == {k: v for k, v in psummary.items() if k != timing}


def test_apply_r_map_on_the_host_route_and_in_pca_space(map_run, tmp_path):
    from ganrev import apply_r
    where, summary, _ = map_run
    host = tmp_path / "host"
    hsummary = apply_r.main(["--synthetic", "3x32x32x32", "--nbImages", "520", "--quiet", "--host", "--map", "--mapIterations", "300", "--writeTo", str(host)])
    for f in MAP_FILES[:3] + ("attributes.npy",):                                       # the uploaded table is the same table: the same map
        assert open(where / f, "rb").read() == open(host / f, "rb").read(), f
    assert hsummary["map"] == summary["map"] and not os.path.exists(host / "map.png")   # no --render: no picture
    space = tmp_path / "space"
    ssummary = apply_r.main(["--synthetic", "3x32x32x32", "--nbImages", "520", "--quiet", "--resident", "--pca", "4", "--pcaSpace", "--map", "--mapRows", "100",
                             "--mapPerplexity", "10", "--mapIterations", "50", "--mapGrid", "4", "--writeTo", str(space)])
    assert ssummary["map"]["space"] == "pca_whitened" and ssummary["map"]["d"] == 4 and ssummary["map"]["rows"] == 100
    assert np.load(space / "map_y.npy").shape == (100, 2) and np.load(space / "map_cells.npy").shape == (4, 4) and np.load(space / "map_cells.npy").max() < 100
