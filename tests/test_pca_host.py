"""not-gpu: the numpy restatement of gr_pca_dev's summation order (tests/pca_paths.py) against float64 (tests/pca_oracle.py) within the bounds
pca_paths derives, on the shapes tests/test_gpu_pca.py runs on the device; the one-pass formula missing that bound far from the origin;
ganrev.pca.axisVariations against a hand-written case; apply_r's option parsing; the header's and the bindings' new symbols."""
import os
import re
import types

import numpy as np
import pytest

import pca_oracle as po
import pca_paths as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_SHAPES = [(2, 5), (511, 5), (512, 5), (513, 5), (512 * (pp.P + 1) + 3, 8)]
COLUMN_SHAPES = [(700, d) for d in (1, 2, 3, 100, 255, 256)]


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(err).all()
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("n,d", ROW_SHAPES + COLUMN_SHAPES)
def test_restated_mean_and_covariance_meet_their_bounds(n, d):
    x = po.gaussian(n, d)
    m = pp.mean(x)
    assert worst(np.abs(m - po.mean(x)), pp.mean_bound(x)) <= 1
    c = pp.covariance(x, m)
    assert np.array_equal(c, c.T)
    ratio = worst(np.abs(c - po.covariance(x)), pp.cov_bound(x))
    print(f"n {n} d {d}: cov err / bound {ratio:.3g}")
    assert ratio <= 1


def test_partial_ranges_cover_the_blocks_once_and_unevenly():
    n = 512 * (pp.P + 1) + 3
    r = pp.partial_ranges(n)
    assert len(r) == pp.P and r[0][0] == 0 and r[-1][1] == pp.blocks(n) == pp.P + 2
    assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert sorted({hi - lo for lo, hi in r}) == [1, 2]                   # a workgroup that owns more than one block, and ranges that differ
    assert sum(hi == lo for lo, hi in pp.partial_ranges(700)) == pp.P - 2     # two blocks: every other partial is empty


def test_far_from_the_origin_the_bound_holds_and_one_pass_misses_it():
    x = po.far_from_origin(700, 6)
    ref, bound = po.covariance(x), pp.cov_bound(x)
    assert worst(np.abs(pp.covariance(x, pp.mean(x)) - ref), bound) <= 1
    miss = worst(np.abs(po.one_pass_f32(x) - ref), bound)
    print(f"one-pass float32: err / bound {miss:.3g}")
    assert miss > 100                                                    # orders of magnitude: the case bites


@pytest.mark.parametrize("n,d,k,whiten", [(300, 7, 1, False), (300, 7, 7, True), (130, 100, 100, False)])
def test_restated_projection_meets_its_bound(n, d, k, whiten):
    x = po.gaussian(n, d)
    m = pp.mean(x)
    w, axes = po.eigh_descending(po.covariance(x))
    axes = axes.astype(np.float32)
    if whiten:
        w = w.copy(); w[-1] = 0.0
    ref, scale = po.project(x, m, axes, w, k, whiten)
    got = pp.project(x, m, axes, w, k, whiten)
    assert worst(np.abs(got - ref), pp.project_bound(scale, d)) <= 1
    if whiten:
        assert not got[:, -1].any()


def test_axis_variations_by_hand():
    from ganrev import pca as P
    pca = types.SimpleNamespace(mean=np.array([0.5, -0.25]), eigenvalues=np.array([4.0, -1e-9]), axes=np.array([[0.6, 0.8], [-0.8, 0.6]], np.float32))
    rows = P.axisVariations(pca, 2, 3, "normal")
    assert rows.dtype == np.float32 and rows.shape == (6, 2)
    a0 = np.float64(np.float32(0.6)), np.float64(np.float32(0.8))
    want = [[0.5 - 6 * a0[0], -0.25 - 6 * a0[1]], [0.5, -0.25], [0.5 + 6 * a0[0], -0.25 + 6 * a0[1]],      # t = -3, 0, 3 times sqrt(4)
            [0.5, -0.25], [0.5, -0.25], [0.5, -0.25]]                                                       # a negative eigenvalue: no spread
    assert np.array_equal(rows, np.array(want, np.float64).astype(np.float32))
    clamped = P.axisVariations(pca, 1, 3, "uniform")
    assert np.array_equal(clamped, np.clip(np.array(want[:3]), -1, 1).astype(np.float32)) and clamped.min() == -1 and clamped.max() == 1
    assert np.array_equal(P.explainedRatios([3.0, 1.0, 0.0, -1e-12]), [0.75, 0.25, 0.0, 0.0])
    with pytest.raises(Exception):
        P.axisVariations(pca, 3)


def test_apply_r_refuses_pcaSpace_without_pca_and_more_axes_than_noise_dimensions(capsys):
    from ganrev import apply_r
    ok = apply_r.parse(["--synthetic", "1x32x32x32", "--pca", "32", "--pcaSpace"])
    assert apply_r.pcaOptions(ok) == (32, True)
    plain = apply_r.parse(["--synthetic", "1x32x32x32"])
    assert apply_r.pcaOptions(plain) == (0, False) and not hasattr(plain, "pca") and not hasattr(plain, "pcaSpace")     # off leaves the namespace as it was
    for argv, word in ((["--synthetic", "1x32x32x32", "--pcaSpace"], "--pca K"), (["--synthetic", "1x32x32x32", "--pca", "33"], "noiseDim"),
                       (["--synthetic", "1x32x32x32", "--pca", "-1"], "--pca")):
        with pytest.raises(SystemExit):
            apply_r.parse(argv)
        assert word in capsys.readouterr().err


def test_the_header_and_the_bindings_declare_the_new_symbols():
    from ganrev import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ganrev.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "gan-reverser_amd", "lua", "hipnn.lua")).read()
    for name in ("gr_pca_dev", "gr_pca_project_dev"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in L.EXPORTED_SYMBOLS and name + "(" in lua
    assert hasattr(L.Context, "pca_dev") and hasattr(L.Context, "pca_project_dev")
    src = open(os.path.join(ROOT, "gan-reverser_amd", "csrc", "pca.hip")).read()
    shared = open(os.path.join(ROOT, "gan-reverser_amd", "csrc", "kernels.h")).read()         # ROWS_PER_BLOCK: the one constant of every family
    for text, name, value in ((shared, "ROWS_PER_BLOCK", pp.RPB), (src, "PCA_P", pp.P), (src, "PCA_SWEEP_CAP", pp.SWEEP_CAP), (src, "PCA_DMAX", pp.MAX_D)):
        assert re.search(r"constexpr int " + name + r" = (\d+)", text).group(1) == str(value)     # pca_paths restates the library's constants
    assert "PCA_TAU2 = 0x1p-92" in src and pp.TAU ** 2 == 2.0 ** -92
