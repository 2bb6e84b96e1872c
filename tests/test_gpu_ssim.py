"""gpu: gr_ssim_dev / gr_ssim_host (csrc/quality.hip) against the direct-form float64 oracle (tests/ssim_oracle.py) within the bounds tests/ssim_paths.py
derives from the header's operation chain - every numeric check asserts worst err / bound <= 1 and prints the ratio - the chain's bit-for-bit
identities, its limits, and ganrev.compare and ganrev.apply_r --anomalyMetric ssim end to end.  Outputs start from garbage (7)."""
import contextlib
import json
import os

import numpy as np
import pytest

import ganrev._lib as L
import ssim_oracle as so
import ssim_paths as sp
from ganrev import apply_r, compare
from ganrev import quality as Q
from ganrev.nn_utils import DeviceTensor
from test_ssim_host import check

pytestmark = pytest.mark.gpu

GR_ERR_INVALID = -1        # include/ganrev.h gr_status


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [None if a is None else ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            if p is not None:
                ctx.free(p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(x, y):
    return all((p is None and q is None) or np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))


def ssim_dev(ctx, a, b, win=11, sigma=1.5, data_range=1.0, misalign=False, want=(True, True)):
    """-> (ssim_rows, mse_rows, mean) through gr_ssim_dev; what was not asked for comes back as the garbage it started from.  misalign: both
    tables offset by 4 bytes (the scalar loads whatever w)"""
    n, c, h, w = a.shape
    pad = lambda t: np.concatenate([np.zeros(1, np.float32), t.reshape(-1)]) if misalign else t
    off = 4 if misalign else 0
    outs = (np.full(n, 7, np.float32), np.full(n, 7, np.float32), np.full(1, 7.0))
    with on_device(ctx, pad(a), pad(b), *outs) as (da, db, dr, dm, dq):
        ctx.ssim_dev(da + off, db + off, n, c, h, w, dr, dm if want[0] else None, dq if want[1] else None, win=win, sigma=sigma, data_range=data_range)
        return ctx.download(dr, (n,)), ctx.download(dm, (n,)), float(ctx.download(dq, (1,), np.float64)[0])


# ------------------------------------------------------------------ 1. the kernel against the oracle
MEAN_EDGES = [(n, 1, 3, 3, 3) for n in (512, 4096, 4097)]      # the mean's chain: one full block, eight partials exactly, a ninth (1 and 513 images are in SHAPES)


@pytest.mark.parametrize("shape", so.SHAPES + MEAN_EDGES, ids=str)
def test_ssim_matches_the_oracle_within_the_derived_bounds(ctx, shape):
    for kind in so.KINDS:
        a, b, _, _ = so.case(kind, shape)
        got = ssim_dev(ctx, a, b, win=shape[4])
        check(got, kind, shape, str(shape))
        assert same_bits(ssim_dev(ctx, a, b, win=shape[4]), got), "two runs agree"
        assert same_bits(ssim_dev(ctx, b, a, win=shape[4]), got), "the chain is symmetric"
        assert same_bits(ctx.ssim_host(a, b, win=shape[4]), got), "_host gives the bits of _dev"
        one = ssim_dev(ctx, a, a, win=shape[4])
        assert (one[0] == np.float32(1)).all() and not one[1].any() and one[2] == 1.0, "a == b gives exactly 1 and mse 0"


def test_uniform_window(ctx):
    shape = (2, 3, 33, 17, 7)
    for kind in so.KINDS:
        a, b, _, _ = so.case(kind, shape, 0.0)
        check(ssim_dev(ctx, a, b, win=7, sigma=0.0), kind, shape, "uniform", sigma=0.0)


def test_tables_offset_by_four_bytes_give_the_bits_of_the_aligned_run(ctx):
    shape = (4, 3, 32, 32, 11)
    for kind in so.KINDS:
        a, b, _, _ = so.case(kind, shape)
        got = ssim_dev(ctx, a, b, misalign=True)
        check(got, kind, shape, "misaligned")
        assert same_bits(got, ssim_dev(ctx, a, b))


def test_null_outputs_are_accepted_and_left_alone(ctx):
    a, b, _, _ = so.case("noise", (513, 1, 11, 11, 11))
    full = ssim_dev(ctx, a, b)
    for want in ((False, False), (True, False), (False, True)):
        part = ssim_dev(ctx, a, b, want=want)
        assert np.array_equal(bits(part[0]), bits(full[0]))
        assert np.array_equal(bits(part[1]), bits(full[1])) if want[0] else (part[1] == 7).all()
        assert part[2] == (full[2] if want[1] else 7.0)
    rows, mse, mean = ctx.ssim_host(a, b, want_mse=False, want_mean=False)
    assert mse is None and mean is None and np.array_equal(bits(rows), bits(full[0]))


def test_mean_is_the_block_mean_of_the_rows(ctx):
    """ssim_mean against the contract's own chain on the float rows: within their rounding of it; and exactly 1 past two block edges"""
    for shape in ((513, 1, 11, 11, 11), (1025, 1, 3, 3, 3)):
        a, b, ref, bnd = so.case("noise", shape)
        rows, _, mean = ssim_dev(ctx, a, b, win=shape[4])
        r = rows.astype(np.float64)
        parts = [Q._ordered_sum(r[lo:lo + 512], 0) for lo in range(0, len(r), 512)]
        again = float(Q._ordered_sum(np.array(parts), 0) / len(r))
        assert abs(mean - again) <= sp.U32 * float(np.abs(ref[0]).mean()) * 1.01 + bnd["mean"]
        assert ssim_dev(ctx, a, a, win=shape[4])[2] == 1.0


def test_mse_rows_agree_with_gr_mse_rows_dev(ctx):
    """the squared error of the same pass against the library's per-row criterion: that one subtracts in float (u relative on every difference, 2 u on
    its square), sums in double and rounds once; this one is fp64 throughout and rounds once - within both roundings and the fp64 parts"""
    for shape in ((4, 3, 32, 32, 11), (2, 3, 33, 17, 7)):
        for kind in so.KINDS:
            a, b, ref, bnd = so.case(kind, shape)
            n, per = shape[0], a[0].size
            _, mse, _ = ssim_dev(ctx, a, b, win=shape[4])
            with on_device(ctx, a, b, np.full(n, 7, np.float32)) as (da, db, dl):
                ctx.mse_rows_dev(da, db, n, per, dl)
                other = ctx.download(dl, (n,))
            bound = (4.0 * sp.U32 + sp.gamma(per + 4)) * ref[1] + bnd["mse64"] + sp.TINY32
            ratio = float(np.max(np.abs(mse.astype(np.float64) - other.astype(np.float64)) / bound))
            print(f"{shape} {kind}: mse_rows against gr_mse_rows_dev err / bound = {ratio:.2e}")
            assert ratio <= 1.0


def test_arguments_outside_the_limits_are_refused_before_any_launch(ctx):
    """argument checks of the library itself (the binding's own are bypassed): GR_ERR_INVALID, a message, nothing launched, the context usable"""
    a, b, _, _ = so.case("noise", (3, 1, 5, 9, 3))
    with on_device(ctx, a, b, np.full(3, 7, np.float32)) as (da, db, dr):
        call = lambda n, c, h, w, win, rng, pa=da, pr=dr: ctx.lib.gr_ssim_dev(ctx.h, L._ptr(pa), L._ptr(db), n, c, h, w, win, 1.5, rng, L._ptr(pr), None, None)
        for bad in ((3, 1, 5, 9, 4, 1.0), (3, 1, 5, 9, 1, 1.0), (3, 1, 5, 9, 13, 1.0), (3, 1, 5, 9, 7, 1.0), (3, 1, 9, 5, 7, 1.0), (3, 1, 129, 9, 3, 1.0),
                    (3, 1, 5, 129, 3, 1.0), (3, 1, 5, 9, 3, 0.0), (3, 1, 5, 9, 3, -1.0), (3, 1, 5, 9, 3, float("nan")), (0, 1, 5, 9, 3, 1.0),
                    (2 ** 31, 1, 5, 9, 3, 1.0), (3, 0, 5, 9, 3, 1.0)):
            assert call(*bad) == GR_ERR_INVALID, bad
            assert ctx.lib.gr_last_error(ctx.h)
        assert call(3, 1, 5, 9, 3, 1.0, pa=None) == GR_ERR_INVALID and call(3, 1, 5, 9, 3, 1.0, pr=None) == GR_ERR_INVALID
        assert (ctx.download(dr, (3,)) == 7).all(), "nothing was launched"
        with pytest.raises(L.GanrevError):
            ctx.ssim_dev(da, db, 3, 1, 5, 9, dr, win=4)
        assert call(3, 1, 5, 9, 3, 1.0) == L.GR_OK
        check((ctx.download(dr, (3,)), None, None), "noise", (3, 1, 5, 9, 3), "after the refusals")
    z = np.zeros((2, 1, 8, 8), np.float32)
    for args, kw in (((z, z[:1]), {}), ((z, z), dict(win=11)), ((z, z), dict(win=3, data_range=0.0))):
        with pytest.raises(L.GanrevError):
            ctx.ssim_host(*args, **kw)


def test_quality_ssim_on_device_tensors(ctx):
    a, b, _, _ = so.case("noise", (4, 3, 32, 32, 11))
    ta, tb = DeviceTensor(ctx, a.shape), DeviceTensor(ctx, b.shape)
    try:
        ctx.upload(a, ta.ptr); ctx.upload(b, tb.ptr)
        got = Q.ssim(ta, tb)
        check(got, "noise", (4, 3, 32, 32, 11), "quality.ssim")
        assert same_bits(got[:2], ssim_dev(ctx, a, b)[:2])
        with pytest.raises(L.GanrevError):
            Q.ssim(ta, tb.rows(0, 2))
    finally:
        ta.free(); tb.free()


# ------------------------------------------------------------------ 2. the scripts
@pytest.fixture
def scored(monkeypatch):
    """every (a, b) a script hands to quality.ssim, as host copies in call order"""
    calls, real = [], Q.ssim

    def spy(a, b, **kw):
        calls.append((a.numpy(), b.numpy()))
        return real(a, b, **kw)
    monkeypatch.setattr(Q, "ssim", spy)
    return calls, real


def rescore(ctx, real, pair):
    ta, tb = (DeviceTensor(ctx, t.shape) for t in pair)
    try:
        ctx.upload(pair[0], ta.ptr); ctx.upload(pair[1], tb.ptr)
        return real(ta, tb)
    finally:
        ta.free(); tb.free()


def test_compare_end_to_end(ctx, tmp_path, scored):
    from ganrev import png
    calls, real = scored
    out = str(tmp_path / "cmp")
    summary = compare.main(["--synthetic", "1x32x32x8", "--nbImages", "40", "--batchSize", "16", "--render", "--out", out, "--quiet"])
    on_disk = json.load(open(os.path.join(out, "summary.json")))
    assert on_disk == json.loads(json.dumps(summary)) and len(calls) == 4
    load = lambda exp, pair, m: np.load(os.path.join(out, f"compare_{exp}_{pair}_{m}.npy"))
    for (exp, pair), tables in zip((("own", "a"), ("own", "b"), ("real", "a"), ("real", "b")), calls):
        arrays = {m: load(exp, pair, m) for m in ("ssim", "mse", "psnr")}
        for m, v in arrays.items():
            assert v.shape == (40,) and np.isfinite(v).all(), (exp, pair, m)
        assert tables[0].shape == (40, 1, 32, 32) and not np.array_equal(tables[0], tables[1])
        rows, mse, mean = rescore(ctx, real, tables)                          # quality.ssim on the same tables: bit for bit
        assert np.array_equal(bits(rows), bits(arrays["ssim"])) and np.array_equal(bits(mse), bits(arrays["mse"]))
        assert np.array_equal(arrays["psnr"], Q.psnr(mse))
        assert on_disk[exp][pair]["ssim"]["mean"] == float(arrays["ssim"].astype(np.float64).mean()) and on_disk[exp][pair]["ssim_mean_dev"] == mean
        assert (arrays["ssim"] <= 1).all() and (arrays["mse"] > 0).all()
        check((rows, mse, mean), None, None, f"compare {exp} {pair}", pair=tables)
    assert np.array_equal(calls[2][0], calls[3][0]), "both pairs see the same real images"
    sa, sb, ma, mb = load("real", "a", "ssim"), load("real", "b", "ssim"), load("real", "a", "mse"), load("real", "b", "mse")
    assert on_disk["real"]["a_wins_ssim"] == float((sa > sb).mean()) and on_disk["real"]["a_wins_mse"] == float((ma < mb).mean())
    assert on_disk["real"]["rendered_rows"] == sum(compare.extreme_rows(sa, sb), [])
    pic = png.read_png(os.path.join(out, "compare_real.png"))
    assert pic.shape[:2] == (8 * 32, 12 * 32)                                 # 32 triples, four to a row


def test_apply_r_anomaly_metric_ssim(ctx, tmp_path, scored):
    calls, real = scored
    base = ["--synthetic", "1x32x32x8", "--nbImages", "130", "--resident", "--quiet"]
    dirs = {k: str(tmp_path / k) for k in ("ssim", "dist", "plain")}
    s_ssim = apply_r.main(base + ["--anomalyMetric", "ssim", "--writeTo", dirs["ssim"]])
    s_dist = apply_r.main(base + ["--anomalyMetric", "dist", "--writeTo", dirs["dist"]])
    s_plain = apply_r.main(base + ["--writeTo", dirs["plain"]])
    assert len(calls) == 1 and calls[0][0].shape == (130, 1, 32, 32), "only the run that asks for it scores with SSIM"
    rows, _, _ = rescore(ctx, real, calls[0])
    saved = np.load(os.path.join(dirs["ssim"], "anomaly_ssim.npy"))
    assert saved.shape == (130,) and np.array_equal(bits(saved), bits(rows))
    check((rows, None, None), None, None, "apply_r", pair=calls[0])
    below, flags = apply_r.lowestShare(saved, 0.15)
    assert flags.sum() == 19 and s_ssim["anomalies"] == 19 and s_ssim["anomaly_below"] == float(below) and s_ssim["anomaly_metric"] == "ssim"
    assert s_dist["anomaly_metric"] == "dist" and "anomaly_metric" not in s_plain
    assert not os.path.exists(os.path.join(dirs["dist"], "anomaly_ssim.npy")) and not os.path.exists(os.path.join(dirs["plain"], "anomaly_ssim.npy"))
    # without the flag, and with --anomalyMetric dist, the run writes what it wrote before the option existed
    names = sorted(f for f in os.listdir(dirs["plain"]) if f.endswith(".npy"))
    assert names == sorted(f for f in os.listdir(dirs["dist"]) if f.endswith(".npy")) and "anomaly_distances.npy" in names
    for f in names:
        plain = open(os.path.join(dirs["plain"], f), "rb").read()
        assert plain == open(os.path.join(dirs["dist"], f), "rb").read(), f
        assert plain == open(os.path.join(dirs["ssim"], f), "rb").read(), f  # the distances are still written from dist
    drop = lambda s: {k: v for k, v in s.items() if k not in ("anomaly_metric", "embed_and_search_seconds")}
    assert drop(s_dist) == drop(s_plain)
