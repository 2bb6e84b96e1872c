"""gpu: gr_pca_dev and gr_pca_project_dev (csrc/pca.hip) against float64 numpy (tests/pca_oracle.py) within the bounds tests/pca_paths.py derives from
the library's summation structure - every check asserts max err / bound <= 1 and prints the ratio - and ganrev.apply_r --pca / --pcaSpace.
A run of apply_r without the new options makes the calls it made before: tests/test_gpu_apply_r_resident.py, test_gpu_embed.py and
test_gpu_imagegrid.py hold those files; here the files of a run with --pca are compared with those of the same run without it."""
import contextlib
import json
import os
import struct

import numpy as np
import pytest

import pca_oracle as po
import pca_paths as pp

pytestmark = pytest.mark.gpu
ROW_SHAPES = [(2, 5), (511, 5), (512, 5), (513, 5), (512 * (pp.P + 1) + 3, 8)]
COLUMN_SHAPES = [(700, d) for d in (1, 2, 3, 100, 255, 256)]


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
    assert np.isfinite(err).all()
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def pca_dev(ctx, x, want_cov=True):
    """-> (mean f64 [d], cov f64 [d, d] or None, eigenvalues f64 [d], axes f32 [d, d], sweeps, converged); the outputs start from garbage"""
    n, d = x.shape
    outs = (np.full(d, 7.0), np.full((d, d), 7.0), np.full(d, 7.0), np.full((d, d), 7, np.float32), np.full(2, 7, np.int32))
    with on_device(ctx, x, *outs) as (dx, dm, dc, de, da, di):
        ctx.pca_dev(dx, n, d, dm, dc if want_cov else None, de, da, di)
        info = ctx.download(di, (2,), np.int32)
        return (ctx.download(dm, (d,), np.float64), ctx.download(dc, (d, d), np.float64) if want_cov else None, ctx.download(de, (d,), np.float64),
                ctx.download(da, (d, d)), int(info[0]), int(info[1]))


def project_dev(ctx, x, mean, axes, eigenvalues, k, whiten, misalign=False):
    n, d = x.shape
    table = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]) if misalign else x
    with on_device(ctx, table, np.asarray(mean, np.float64), np.asarray(axes, np.float32), np.asarray(eigenvalues, np.float64),
                   np.full((n, k), 7, np.float32)) as (dx, dm, da, de, do):
        ctx.pca_project_dev(dx + 4 if misalign else dx, n, d, dm, da, de, k, whiten, do)
        return ctx.download(do, (n, k))


# ------------------------------------------------------------------ 1. mean and covariance
@pytest.mark.parametrize("n,d", ROW_SHAPES + COLUMN_SHAPES)
def test_mean_and_covariance(ctx, n, d):
    x = po.gaussian(n, d)
    mean, cov, _, _, _, _ = pca_dev(ctx, x)
    rm = worst(np.abs(mean - po.mean(x)), pp.mean_bound(x))
    rc = worst(np.abs(cov - po.covariance(x)), pp.cov_bound(x))
    print(f"n {n} d {d}: mean err / bound {rm:.3g}, cov err / bound {rc:.3g}")
    assert rm <= 1 and rc <= 1
    assert np.array_equal(cov.view(np.uint64), cov.T.copy().view(np.uint64))            # both triangles, bit for bit


@pytest.mark.parametrize("n,d", [(513, 5), (700, 100), (512 * (pp.P + 1) + 3, 8)])
def test_mean_and_covariance_have_the_restated_bits(ctx, n, d):
    x = po.gaussian(n, d)
    mean, cov, _, _, _, _ = pca_dev(ctx, x)
    rmean = pp.mean(x)
    assert np.array_equal(mean.view(np.uint64), rmean.view(np.uint64))
    assert np.array_equal(cov.view(np.uint64), pp.covariance(x, rmean).view(np.uint64))


def test_far_from_the_origin(ctx):
    x = po.far_from_origin(700, 6)
    ref, bound = po.covariance(x), pp.cov_bound(x)
    _, cov, _, _, _, _ = pca_dev(ctx, x)
    ratio, miss = worst(np.abs(cov - ref), bound), worst(np.abs(po.one_pass_f32(x) - ref), bound)
    print(f"mean 1000, sd 1: cov err / bound {ratio:.3g}; the float32 one-pass formula {miss:.3g}")
    assert ratio <= 1
    assert miss > 100                                                                   # the case bites: a one-pass kernel fails it by orders of magnitude


# ------------------------------------------------------------------ 2. the eigen-solver, against eigh of the covariance the library itself wrote
MATRICES = {
    "d1": lambda: po.gaussian(50, 1), "d2": lambda: po.gaussian(50, 2), "d3": lambda: po.gaussian(200, 3), "d255": lambda: po.gaussian(700, 255),
    "d256": lambda: po.gaussian(700, 256), "diagonal": lambda: po.independent_columns(6), "constant_column": lambda: po.with_constant_column(300, 8),
    "isotropic": lambda: po.isotropic(2000, 16), "rank_deficient": lambda: po.gaussian(5, 16), "geometric_d100": lambda: po.geometric_spectrum(2000, 100),
}
GAPPED = ("d2", "d3", "geometric_d100")                                                 # spectra with gaps: the vectors themselves are compared


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_eigen_solver(ctx, name):
    x = MATRICES[name]()
    d = x.shape[1]
    mean, cov, lam, axes, sweeps, converged = pca_dev(ctx, x)
    assert converged == 1 and 0 <= sweeps <= pp.SWEEP_CAP
    assert np.isfinite(lam).all() and np.isfinite(axes).all() and np.isfinite(cov).all()
    assert (np.diff(lam) <= 0).all()                                                    # descending
    assert po.sign_rule_holds(axes)
    w, v = po.eigh_descending(cov)
    v64 = axes.astype(np.float64)
    r_lam = worst(np.abs(lam - w), np.full(d, pp.eigenvalue_bound(cov, sweeps)))
    res = np.linalg.norm(cov @ v64.T - v64.T * lam[None, :], axis=0)
    r_res = worst(res, np.full(d, pp.residual_bound(cov, sweeps)))
    r_orth = worst(np.abs(v64 @ v64.T - np.eye(d)), np.full((d, d), pp.orthogonality_bound(d, sweeps)))
    print(f"{name}: d {d}, sweeps {sweeps}; eigenvalues err / bound {r_lam:.3g}, residual {r_res:.3g}, orthogonality {r_orth:.3g}")
    if np.linalg.norm(cov) > 0:
        assert r_lam <= 1 and r_res <= 1
    else:
        assert not lam.any()
    assert r_orth <= 1
    if name == "diagonal":
        assert sweeps == 0 and np.array_equal(lam, np.sort(np.diag(cov))[::-1]) and np.array_equal(axes, np.eye(d, dtype=np.float32))
    if name == "constant_column":
        assert not cov[2].any() and not cov[:, 2].any() and np.abs(lam).min() <= pp.eigenvalue_bound(cov, sweeps)
    if name in GAPPED:
        flip = np.sign(np.sum(v64 * v, axis=1))
        dist = np.linalg.norm(v64 - flip[:, None] * v, axis=1)
        r_vec = worst(dist, pp.vector_bound(cov, sweeps, w))
        print(f"{name}: vectors err / bound {r_vec:.3g}")
        assert r_vec <= 1


def test_without_the_covariance_output_the_rest_is_the_same(ctx):
    x = po.gaussian(513, 5)
    a, b = pca_dev(ctx, x), pca_dev(ctx, x, want_cov=False)
    assert b[1] is None
    for u, v in zip(a[:1] + a[2:4], b[:1] + b[2:4]):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert a[4:] == b[4:]


# ------------------------------------------------------------------ 3. projection
PROJECTIONS = {           # name: (n, d, k, whiten, misaligned pointer)
    "k1": (300, 7, 1, False, False), "kd_odd_d": (300, 7, 7, False, False), "whiten": (300, 7, 7, True, False), "vector_loads": (130, 100, 100, False, False),
    "misaligned": (130, 100, 100, False, True), "d256_two_axis_tiles": (700, 256, 256, True, False),
}


@pytest.mark.parametrize("name", sorted(PROJECTIONS))
def test_projection(ctx, name):
    n, d, k, whiten, misalign = PROJECTIONS[name]
    x = po.gaussian(n, d)
    w, axes = po.eigh_descending(po.covariance(x))
    axes, w, mean = axes.astype(np.float32), w.copy(), po.mean(x)
    if whiten:
        w[-1], w[-2] = 0.0, -1e-3                                                      # not positive: a zero column each
    got = project_dev(ctx, x, mean, axes, w, k, whiten, misalign)
    ref, scale = po.project(x, mean, axes, w, k, whiten)
    ratio = worst(np.abs(got - ref), pp.project_bound(scale, d))
    print(f"{name}: n {n} d {d} k {k} whiten {whiten}: err / bound {ratio:.3g}")
    assert ratio <= 1
    if whiten:
        assert not got[:, -2:].any() and got[:, :-2].any()
    assert np.array_equal(got.view(np.uint32), pp.project(x, mean, axes, w, k, whiten).view(np.uint32))      # the restated chain, bit for bit


# ------------------------------------------------------------------ 4. determinism, limits
def test_two_runs_agree_bit_for_bit(ctx):
    x = po.gaussian(3000, 33)
    a, b = pca_dev(ctx, x), pca_dev(ctx, x)
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert a[4:] == b[4:]
    p = [project_dev(ctx, x, a[0], a[3], a[2], 33, True) for _ in range(2)]
    assert np.array_equal(p[0].view(np.uint32), p[1].view(np.uint32))


def test_limits(ctx):
    import ganrev._lib as L
    x = po.gaussian(513, 5)
    big = np.zeros((8, 257), np.float32)
    with on_device(ctx, big, np.zeros(257), np.zeros((257, 257)), np.zeros(257), np.zeros((257, 257), np.float32), np.zeros(2, np.int32),
                   np.zeros((8, 257), np.float32)) as (dx, dm, dc, de, da, di, do):
        for (n, d), code, word in (((8, 257), "GR_ERR_UNSUPPORTED", "257"), ((1, 5), "GR_ERR_UNSUPPORTED", "n 1"), ((0, 5), "GR_ERR_INVALID", "n 0"),
                                   ((8, 0), "GR_ERR_INVALID", "d 0")):
            with pytest.raises(L.GanrevError, match=code) as e:
                ctx.pca_dev(dx, n, d, dm, dc, de, da, di)
            assert word in str(e.value), str(e.value)
        for args in ((None, dm, dc, de, da, di), (dx, None, dc, de, da, di), (dx, dm, dc, None, da, di), (dx, dm, dc, de, None, di), (dx, dm, dc, de, da, None)):
            with pytest.raises(L.GanrevError, match="GR_ERR_INVALID") as e:                # (cov_dev is the one nullable pointer)
                ctx.pca_dev(args[0], 8, 5, *args[1:])
            assert "null pointer" in str(e.value)
        for (n, d, k), code, word in (((8, 5, 0), "GR_ERR_INVALID", "k 0"), ((8, 5, 6), "GR_ERR_UNSUPPORTED", "k 6"), ((8, 257, 4), "GR_ERR_UNSUPPORTED", "257"),
                                      ((0, 5, 2), "GR_ERR_INVALID", "n 0")):
            with pytest.raises(L.GanrevError, match=code) as e:
                ctx.pca_project_dev(dx, n, d, dm, da, de, k, 1, do)
            assert word in str(e.value), str(e.value)
        for args in ((None, dm, da, de, do), (dx, None, da, de, do), (dx, dm, None, de, do), (dx, dm, da, None, do), (dx, dm, da, de, None)):
            with pytest.raises(L.GanrevError, match="GR_ERR_INVALID") as e:
                ctx.pca_project_dev(args[0], 8, 5, args[1], args[2], args[3], 2, 1, args[4])
            assert "null pointer" in str(e.value)
        ctx.pca_project_dev(dx, 8, 5, dm, da, None, 2, 0, do)                           # the eigenvalues are not read without whitening
    mean, cov, lam, axes, sweeps, converged = pca_dev(ctx, x)                           # the context stays usable
    assert converged == 1 and worst(np.abs(cov - po.covariance(x)), pp.cov_bound(x)) <= 1


# ------------------------------------------------------------------ 5. the script
BASE = ["--synthetic", "3x32x32x32", "--nbImages", "600", "--quiet"]
PCA_FILES = ("pca_mean.npy", "pca_eigenvalues.npy", "pca_axes.npy", "pca_projection.npy")


def run_apply_r(tmp, name, *options):
    from ganrev import apply_r
    where = tmp / name
    summary = apply_r.main(BASE + list(options) + ["--writeTo", str(where)])
    return where, summary


def png_size(path):
    head = open(path, "rb").read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", head[16:24])


@pytest.fixture(scope="module")
def resident_run(tmp_path_factory):
    return run_apply_r(tmp_path_factory.mktemp("pca"), "resident", "--pca", "4", "--render", "--resident")


def test_apply_r_pca_writes_its_files(ctx, resident_run):
    import ganrev._lib as L
    from ganrev import pca as P
    where, summary = resident_run
    mean, lam, axes, proj = (np.load(where / f) for f in PCA_FILES)
    assert (mean.shape, mean.dtype, lam.shape, lam.dtype) == ((32,), np.float64, (32,), np.float64)
    assert (axes.shape, axes.dtype, proj.shape, proj.dtype) == ((4, 32), np.float32, (600, 4), np.float32)
    entry = json.load(open(where / "summary.json"))["pca"]
    assert entry == summary["pca"] and entry["k"] == 4 and entry["converged"] is True and 0 <= entry["sweeps"] <= pp.SWEEP_CAP and entry["space"] == "attributes"
    assert len(entry["explained"]) == 4 and entry["explained"] == sorted(entry["explained"], reverse=True) and 0 < sum(entry["explained"]) <= 1 + 1e-12
    _, gh, gw = L.grid_shape(4 * 16, 1, 3, 32, 32, -1, 16)
    assert png_size(where / "variations_pca.png") == (gw, gh) and png_size(where / "variations.png") == (gw, 8 * gh)      # 4 and 32 rows of 16 steps
    attrs = np.load(where / "attributes.npy")
    with on_device(ctx, attrs) as (da,):                                                # the files are what the package computes on that table
        pca = P.principalAxes(ctx, da, 600, 32)
        try:
            t = P.project(ctx, pca, da, 600, 4)
            again = t.numpy(); t.free()
            assert np.array_equal(pca.mean, mean) and np.array_equal(pca.eigenvalues, lam) and np.array_equal(pca.axes[:4], axes)
            assert np.array_equal(again.view(np.uint32), proj.view(np.uint32))
            assert entry["explained"] == [float(v) for v in pca.explained[:4]]
        finally:
            pca.close()
    ref, scale = po.project(attrs, mean, axes, lam, 4, False)
    assert worst(np.abs(proj - ref), pp.project_bound(scale, 32)) <= 1


def test_apply_r_host_route_gives_the_same_bytes(resident_run, tmp_path):
    where, summary = resident_run
    host, hsummary = run_apply_r(tmp_path, "host", "--pca", "4", "--render", "--host")
    for f in PCA_FILES + ("attributes.npy",):
        assert open(where / f, "rb").read() == open(host / f, "rb").read(), f
    assert hsummary["pca"] == summary["pca"] and os.path.exists(host / "variations_pca.png")


def test_apply_r_without_pca_writes_the_same_files(resident_run, tmp_path):
    where, summary = resident_run
    plain, psummary = run_apply_r(tmp_path, "plain", "--render", "--resident")
    names = sorted(os.listdir(plain))
    assert "pca" not in psummary and not [f for f in names if "pca" in f]
    assert sorted(os.listdir(where)) == sorted(names + list(PCA_FILES) + ["variations_pca.png"])
    for f in names:
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(where / f, "rb").read(), f
    timing = "embed_and_search_seconds"
    assert {k: v for k, v in summary.items() if k not in ("pca", timing)} == {k: v for k, v in psummary.items() if k != timing}


def test_apply_r_pcaSpace_on_the_route_that_copies_the_tables_to_the_host(tmp_path):
    """neither --resident nor --host: the search runs on the device table, the clustering on the host copy of the whitened projection"""
    copied, csummary = run_apply_r(tmp_path, "copied", "--pca", "4", "--pcaSpace")
    resident, rsummary = run_apply_r(tmp_path, "resident", "--pca", "4", "--pcaSpace", "--resident")
    assert csummary["pca"] == rsummary["pca"] and csummary["pca"]["space"] == "pca_whitened"
    for f in PCA_FILES + ("attributes.npy", "similar_by_attributes.npy", "similar_by_pixels.npy"):
        assert open(copied / f, "rb").read() == open(resident / f, "rb").read(), f
    assert np.load(copied / "cluster_centroids.npy").shape == (20, 4) and csummary["cluster_total_counts"] == rsummary["cluster_total_counts"]
    assert not os.path.exists(copied / "variations_pca.png")                            # no --render: no picture


def test_apply_r_pcaSpace_hands_on_the_whitened_projection(ctx, tmp_path, monkeypatch):
    from ganrev import apply_r
    from ganrev import pca as P
    seen = {}
    search, cluster = apply_r.createSimilaritySearchDev, apply_r.createClusterImagesDev

    def spy_search(nbSimilarNeedles, nbShowMax, attributes, images=None):
        seen["search"] = attributes.numpy()
        return search(nbSimilarNeedles, nbShowMax, attributes, images)

    def spy_cluster(nbClusters, nbIterations, nbMaxPerCluster, images, attributes, **kw):
        seen["cluster"] = attributes.numpy()
        return cluster(nbClusters, nbIterations, nbMaxPerCluster, images, attributes, **kw)
    monkeypatch.setattr(apply_r, "createSimilaritySearchDev", spy_search)
    monkeypatch.setattr(apply_r, "createClusterImagesDev", spy_cluster)
    where, summary = run_apply_r(tmp_path, "space", "--pca", "4", "--pcaSpace", "--resident")
    assert summary["pca"]["space"] == "pca_whitened" and json.load(open(where / "summary.json"))["pca"]["space"] == "pca_whitened"
    attrs = np.load(where / "attributes.npy")
    with on_device(ctx, attrs) as (da,):
        pca = P.principalAxes(ctx, da, 600, 32)
        try:
            t = P.project(ctx, pca, da, 600, 4, whiten=True)
            white = t.numpy(); t.free()
        finally:
            pca.close()
    assert white.shape == (600, 4)
    for who in ("search", "cluster"):
        assert np.array_equal(seen[who].view(np.uint32), white.view(np.uint32)), who
    assert np.load(where / "similar_by_attributes.npy").shape == (5, 100) and np.load(where / "cluster_centroids.npy").shape == (20, 4)
    assert np.load(where / "attributes.npy").shape == (600, 32) and np.load(where / "pca_projection.npy").shape == (600, 4)
    sd = white.astype(np.float64).std(axis=0, ddof=1)                                   # whitened: unit variance along every axis
    assert np.abs(sd - 1).max() <= 1e-4
