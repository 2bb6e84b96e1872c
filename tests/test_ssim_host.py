"""not-gpu: the numpy twin of gr_ssim_dev's chain (ganrev.quality.ssim_twin) against the direct-form float64 oracle (tests/ssim_oracle.py) within
the bounds tests/ssim_paths.py derives, the cap on those bounds, the chain's identities, psnr, and the option and argument checks of
ganrev.compare, ganrev.apply_r --anomalyMetric and the bindings that need no GPU."""
import numpy as np
import pytest

import ganrev._lib as L
import ssim_oracle as so
import ssim_paths as sp
from ganrev import apply_r, compare
from ganrev import quality as Q

HOST_SHAPES = [s for s in so.SHAPES if s[0] * s[1] * s[2] * s[3] <= 2 * 3 * 64 * 64]      # the cap case runs on the GPU side; its bound is checked below


def check(got, kind, shape, name, sigma=1.5, pair=None):
    """assert worst err / bound <= 1 for every output given, print the ratios; pair = (a, b): tables of no case (window 11, sigma 1.5)"""
    if pair is not None:
        ref, bnd = so.ssim(*pair), sp.bounds(pair[0], pair[1], 11)
    else:
        _, _, ref, bnd = so.case(kind, shape, sigma)
    r = sp.ratios(got, ref, bnd)
    print(f"{name} {kind}: " + ", ".join(f"{k} err / bound = {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (name, kind, r)
    return r


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_twin_matches_the_oracle_within_the_derived_bounds(shape):
    for kind in so.KINDS:
        a, b, _, _ = so.case(kind, shape)
        check(Q.ssim_twin(a, b, win=shape[4]), kind, shape, str(shape))


def test_twin_with_the_uniform_window():
    shape = (2, 3, 33, 17, 7)
    for kind in so.KINDS:
        a, b, _, _ = so.case(kind, shape, 0.0)
        check(Q.ssim_twin(a, b, win=7, sigma=0.0), kind, shape, "uniform", sigma=0.0)


@pytest.mark.parametrize("shape", so.SHAPES, ids=str)
def test_the_fp64_part_of_every_bound_is_under_the_cap(shape):
    for kind in so.KINDS:
        _, _, _, bnd = so.case(kind, shape)
        worst = max(float(bnd["rows64"].max()), float(bnd["mse64"].max()), bnd["mean64"])
        print(f"{shape} {kind}: fp64 part {worst:.3e}")
        assert worst <= sp.CAP, (shape, kind, worst)


def test_a_float32_twin_fails_the_bound_on_the_flat_kind():
    """the bound tells a float implementation of the window sums from the contract's: on flat images (and on bright low-contrast ones)
    sum w x^2 - mu^2 in float loses 1e-5 and more of the index"""
    for kind in ("constants", "cancellation"):
        shape = (4, 3, 32, 32, 11)
        a, b, ref, bnd = so.case(kind, shape)
        r = sp.ratios(Q.ssim_twin(a, b, dtype=np.float32), ref, bnd)
        print(f"float32 twin, {kind}: rows err / bound = {r['rows']:.1f}")
        assert r["rows"] > 10.0


def test_identities_of_the_chain():
    for kind in ("noise", "cancellation", "constants"):
        a, b, _, _ = so.case(kind, (3, 3, 11, 12, 11))
        rows, mse, mean = Q.ssim_twin(a, a)
        assert (rows == np.float32(1)).all() and not mse.any() and mean == 1.0, "a == b gives exactly 1"
        fwd, rev = Q.ssim_twin(a, b), Q.ssim_twin(b, a)
        assert np.array_equal(fwd[0], rev[0]) and np.array_equal(fwd[1], rev[1]) and fwd[2] == rev[2], "the chain is symmetric"
    a, b, ref, _ = so.case("black_white", (4, 3, 32, 32, 11))
    c1 = 1e-4
    assert abs(ref[0][0] - c1 / (1 + c1)) < 1e-12 and (ref[1] == 1).all()
    _, _, ref, _ = so.case("negative", (4, 3, 32, 32, 11))
    assert (ref[0] < 0).all()


def test_window():
    g = Q.window(11, 1.5)
    assert abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert np.allclose(np.outer(g, g), so.window2d(11, 1.5), rtol=1e-14, atol=0)
    assert np.array_equal(Q.window(7, 0.0), np.full(7, 1.0 / 7))


def test_psnr():
    p = Q.psnr(np.array([0.0, 1.0, 0.01, 0.25], np.float32))
    assert np.isinf(p[0]) and p[0] > 0 and p[1] == 0.0 and abs(p[2] - 20.0) < 1e-5 and abs(p[3] - 10 * np.log10(4.0)) < 1e-12
    assert abs(Q.psnr(np.array([1.0]), data_range=255.0)[0] - 20 * np.log10(255.0)) < 1e-12
    assert Q.psnr(np.zeros((2, 3))).shape == (2, 3)


def test_argument_checks_that_need_no_gpu():
    L.ssim_check_args(1, 1, 3, 3, 3, 1.0)
    L.ssim_check_args(2 ** 31 - 1, 3, 128, 128, 11, 255.0)
    for bad in ((1, 1, 32, 32, 10, 1.0), (1, 1, 32, 32, 13, 1.0), (1, 1, 32, 32, 1, 1.0), (1, 1, 9, 32, 11, 1.0), (1, 1, 32, 9, 11, 1.0),
                (1, 1, 129, 32, 11, 1.0), (1, 1, 32, 129, 11, 1.0), (0, 1, 32, 32, 11, 1.0), (2 ** 31, 1, 32, 32, 11, 1.0), (1, 0, 32, 32, 11, 1.0),
                (1, 1, 32, 32, 11, 0.0), (1, 1, 32, 32, 11, -1.0), (1, 1, 32, 32, 11, float("nan"))):
        with pytest.raises(L.GanrevError):
            L.ssim_check_args(*bad)
    z = np.zeros((2, 1, 8, 8), np.float32)
    with pytest.raises(L.GanrevError):
        Q.ssim_twin(z, z[:1], win=3)
    with pytest.raises(L.GanrevError):
        Q.ssim_twin(z[0], z[0], win=3)
    with pytest.raises(L.GanrevError):
        Q.ssim_twin(z, z, win=11)
    s = Q.score_summary(np.arange(101.0))
    assert s == dict(mean=50.0, median=50.0, p05=5.0, p95=95.0)


def test_compare_options():
    o = compare.parse([])
    assert (o.G, o.R) == (apply_r.parse([]).G, apply_r.parse([]).R)
    assert (o.vaeG, o.vaeR) == ("logs/vae_3x32x32_nd100.net", "logs/vae_r_3x32x32_nd100.net")
    assert (o.win, o.sigma, o.dataset, o.render) == (11, 1.5, "NONE", False)
    o = compare.parse(["--synthetic", "1x32x32x8", "--nbImages", "40", "--batchSize", "16", "--render", "--out", "x"])
    assert (o.synthetic, o.nbImages, o.batchSize, o.render, o.out) == ("1x32x32x8", 40, 16, True, "x")
    for bad in (["--nbImages", "0"], ["--batchSize", "0"], ["--synthetic", "1x32x32"], ["--synthetic", "1x8x8x4"], ["--synthetic", "1x256x256x4"],
                ["--win", "4"], ["--win", "13"], ["--render", "--nbImages", "31"]):
        with pytest.raises(SystemExit):
            compare.parse(bad)
    assert compare.a_wins_share(np.array([0.5, 0.2, 0.9, 0.3]), np.array([0.4, 0.2, 0.1, 0.7])) == 0.5
    assert compare.extreme_rows(np.array([0.1, 0.9, 0.5, 0.3]), np.array([0.2, 0.1, 0.5, 0.9]), 1) == ([1], [3])


def test_apply_r_anomaly_metric_options():
    assert not hasattr(apply_r.parse([]), "anomalyMetric")
    assert apply_r.anomalyMetric(apply_r.parse([])) == "dist"
    assert apply_r.parse(["--resident", "--anomalyMetric", "dist"]).anomalyMetric == "dist"
    assert apply_r.anomalyMetric(apply_r.parse(["--resident", "--anomalyMetric", "ssim"])) == "ssim"
    assert apply_r.parse(["--render", "--anomalyMetric", "ssim"]).anomalyMetric == "ssim"
    for bad in (["--host", "--anomalyMetric", "ssim"], ["--anomalyMetric", "ssim"], ["--resident", "--anomalyMetric", "psnr"],
                ["--resident", "--anomalyMetric", "ssim", "--synthetic", "1x8x8x4"]):
        with pytest.raises(SystemExit):
            apply_r.parse(bad)
    # the reference's index rule on any score: the floor(n * 0.15)-th lowest value, and everything at or below it
    score = np.array([0.9, 0.1, 0.5, 0.3, 0.7, 0.2, 0.8, 0.4, 0.6, 1.0])
    below, flags = apply_r.lowestShare(score, 0.15)
    assert below == 0.1 and flags.tolist() == [False, True] + [False] * 8
    below, flags = apply_r.lowestShare(np.arange(130.0), 0.15)
    assert below == 18.0 and flags.sum() == 19
