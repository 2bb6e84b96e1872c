"""gpu: gr_mixture_dev (csrc/mixture.hip) against float64 numpy (tests/mixture_oracle.py) within the bounds tests/mixture_paths.py derives from the
library's operation chains - every numeric check asserts max err / bound <= 1 and prints the ratio - the member lists above 32 components
(gr_cluster_members_wide_dev) and ganrev.apply_r --mixture.  One E-step and one M-step are each compared from the same float inputs, so no
error propagates; outputs start from garbage (7)."""
import contextlib
import json
import os
import struct

import numpy as np
import pytest

import mixture_oracle as mo
import mixture_paths as mp
import pca_paths as pp
from test_mixture_host import COLUMN_SHAPES, COMPONENT_SHAPES, ROW_SHAPES, case, check_e_step, check_m_step, worst

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


def mixture_dev(ctx, x, w, mu, var, niter, var_floor, rows=(True, True, True), misalign=False):
    """-> dict(weights, means, variances, loglik [niter + 1], labels, post, rowll (None where not asked for))"""
    n, d = x.shape
    k = len(w)
    table = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]) if misalign else x
    outs = (np.full(niter + 1, 7.0), np.full(n, 7, np.int32), np.full(n, 7, np.float32), np.full(n, 7, np.float32))
    with on_device(ctx, table, np.asarray(w, np.float32), np.asarray(mu, np.float32), np.asarray(var, np.float32), *outs) as (dx, dw, dm, dv, dl, dlab, dpost, drow):
        ctx.mixture_dev(dx + 4 if misalign else dx, n, d, k, niter, var_floor, dw, dm, dv, dl, dlab if rows[0] else None, dpost if rows[1] else None,
                        drow if rows[2] else None)
        return dict(weights=ctx.download(dw, (k,)), means=ctx.download(dm, (k, d)), variances=ctx.download(dv, (k, d)),
                    loglik=ctx.download(dl, (niter + 1,), np.float64), labels=ctx.download(dlab, (n,), np.int32), post=ctx.download(dpost, (n,)),
                    rowll=ctx.download(drow, (n,)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_parameters(a, b):
    return all(np.array_equal(bits(a[q]), bits(b[q])) for q in ("weights", "means", "variances"))


def both_steps(ctx, n, d, k, misalign=False):
    x, w, mu, var, floor = case(n, d, k)
    name = f"({n}, {d}, {k})" + (" misaligned" if misalign else "")
    e = mixture_dev(ctx, x, w, mu, var, 0, floor, misalign=misalign)
    assert same_parameters(e, dict(weights=w, means=mu, variances=var))
    check_e_step(dict(rowll=e["rowll"], labels=e["labels"], post=e["post"], loglik=float(e["loglik"][0])), x, w, mu, var, name)
    m = mixture_dev(ctx, x, w, mu, var, 1, floor, misalign=misalign)
    assert m["loglik"][0] == e["loglik"][0]                             # the first E-step is the same E-step
    check_m_step((m["weights"], m["means"], m["variances"]), x, w, mu, var, floor, name)


# ------------------------------------------------------------------ 1. one E-step and one M-step against the oracle
@pytest.mark.parametrize("n,d,k", ROW_SHAPES + COLUMN_SHAPES + COMPONENT_SHAPES)
def test_one_e_step_and_one_m_step(ctx, n, d, k):
    both_steps(ctx, n, d, k)


@pytest.mark.parametrize("n", [1, 4096, 4097])
def test_loglik_at_the_edges_of_its_chain(ctx, n):
    """one row, eight block partials exactly, a ninth (512 and 513 rows are in ROW_SHAPES): the closing E-step alone against the oracle"""
    x, w, mu, var, floor = case(n, 1, 1)
    e = mixture_dev(ctx, x, w, mu, var, 0, floor)
    check_e_step(dict(rowll=e["rowll"], labels=e["labels"], post=e["post"], loglik=float(e["loglik"][0])), x, w, mu, var, f"({n}, 1, 1)")


def test_table_pointer_offset_by_four_bytes(ctx):
    both_steps(ctx, 700, 100, 3, misalign=True)
    x, w, mu, var, floor = case(700, 100, 3)
    a, b = mixture_dev(ctx, x, w, mu, var, 1, floor), mixture_dev(ctx, x, w, mu, var, 1, floor, misalign=True)
    assert same_parameters(a, b) and np.array_equal(bits(a["rowll"]), bits(b["rowll"]))      # the scalar loads read the same values


# ------------------------------------------------------------------ 2. rules
def test_a_dead_component_keeps_mean_and_variances_bit_for_bit(ctx):
    x, _ = mo.blobs(400, 3, 2, seed=4)
    w, mu, var = mo.start(x, np.concatenate([x[:2], np.full((1, 3), 1e4, np.float32)]))
    var[2] = 0.01                                                       # narrow and far: less than one row's worth of responsibility
    got = mixture_dev(ctx, x, w, mu, var, 1, 1e-6)
    assert got["weights"][2] == 0 and np.array_equal(bits(got["means"][2]), bits(mu[2])) and np.array_equal(bits(got["variances"][2]), bits(var[2]))
    assert not np.array_equal(got["means"][:2], mu[:2]) and abs(float(got["weights"].astype(np.float64).sum()) - 1) <= 3 * mp.U32
    again = mixture_dev(ctx, x, got["weights"], got["means"], got["variances"], 2, 1e-6)     # weight 0: l = -inf, and the rest stays finite
    assert again["weights"][2] == 0 and np.array_equal(bits(again["means"][2]), bits(mu[2])) and np.array_equal(bits(again["variances"][2]), bits(var[2]))
    assert np.isfinite(again["loglik"]).all() and np.isfinite(again["rowll"]).all() and not (again["labels"] == 2).any()


def test_the_floor_binds_on_duplicated_rows(ctx):
    row = np.array([[0.5, -1.25, 3.0]], np.float32)
    x = np.repeat(row, 300, axis=0)
    floor = np.float32(0.0625)
    got = mixture_dev(ctx, x, np.ones(1, np.float32), row + np.float32(0.25), np.ones((1, 3), np.float32), 1, floor)
    assert np.array_equal(got["variances"], np.full((1, 3), floor, np.float32))
    assert np.array_equal(got["means"], row) and got["weights"][0] == 1


def test_no_iteration_scores_rows_and_null_outputs_are_accepted(ctx):
    x, w, mu, var, floor = case(513, 5, 2)
    full = mixture_dev(ctx, x, w, mu, var, 0, floor)
    assert same_parameters(full, dict(weights=w, means=mu, variances=var))
    assert not (full["labels"] == 7).any() and not (full["post"] == 7).any() and not (full["rowll"] == 7).any() and full["loglik"][0] != 7
    none = mixture_dev(ctx, x, w, mu, var, 0, floor, rows=(False, False, False))
    assert (none["labels"] == 7).all() and (none["post"] == 7).all() and (none["rowll"] == 7).all() and none["loglik"][0] == full["loglik"][0]
    for rows in ((True, False, False), (False, True, False), (False, False, True)):
        part = mixture_dev(ctx, x, w, mu, var, 1, floor, rows=rows)
        whole = mixture_dev(ctx, x, w, mu, var, 1, floor)
        for q, asked in zip(("labels", "post", "rowll"), rows):
            assert np.array_equal(bits(part[q]), bits(whole[q])) if asked else (part[q] == 7).all()


# ------------------------------------------------------------------ 3. structure
def test_three_iterations_are_three_calls_of_one_and_two_runs_agree(ctx):
    x, w, mu, var, floor = case(1500, 32, 33)
    a, b = mixture_dev(ctx, x, w, mu, var, 3, floor), mixture_dev(ctx, x, w, mu, var, 3, floor)
    for q in a:
        assert np.array_equal(bits(a[q]), bits(b[q])), q
    step, hist = dict(weights=w, means=mu, variances=var), []
    for _ in range(3):
        step = mixture_dev(ctx, x, step["weights"], step["means"], step["variances"], 1, floor)
        hist.append(step["loglik"][0])
    hist.append(step["loglik"][1])
    assert same_parameters(a, step) and np.array_equal(bits(a["loglik"]), bits(np.array(hist)))
    for q in ("labels", "post", "rowll"):
        assert np.array_equal(bits(a[q]), bits(step[q])), q


def test_loglik_does_not_decrease_over_six_iterations(ctx):
    n, d, k = 2000, 100, 20
    x, _ = mo.blobs(n, d, k, seed=2)
    w, mu, var = mo.start(x, x[:k])
    floor = np.float32(1e-6)
    step, bounds = dict(weights=w, means=mu, variances=var), []
    for _ in range(6):                                                  # (the bits of one call with niter = 6: see above)
        e = mo.e_step(x, step["weights"], step["means"], step["variances"])
        bounds.append(mp.loglik_bound(e, mp.ell_bound(x, step["weights"], step["means"], step["variances"])))
        step = mixture_dev(ctx, x, step["weights"], step["means"], step["variances"], 1, floor)
    e = mo.e_step(x, step["weights"], step["means"], step["variances"])
    bounds.append(mp.loglik_bound(e, mp.ell_bound(x, step["weights"], step["means"], step["variances"])))
    got = mixture_dev(ctx, x, w, mu, var, 6, floor)
    assert same_parameters(got, step) and (got["variances"] > floor).all()      # the floor never bound: EM's guarantee applies
    ll = got["loglik"]
    slack = np.array([bounds[t] + bounds[t + 1] for t in range(6)])
    print("loglik", ll.tolist(), "largest decrease / bound", float((-(np.diff(ll)) / slack).max()))
    assert (np.diff(ll) >= -slack).all()
    assert ll[-1] > ll[0]


# ------------------------------------------------------------------ 4. limits
def test_limits(ctx):
    import ganrev._lib as L
    x, w, mu, var, floor = case(513, 5, 2)
    big = np.zeros((257, 257), np.float32)
    with on_device(ctx, big, np.ones(257, np.float32), big + 1, big + 1, np.zeros(8), np.zeros(600, np.int32), np.zeros(600, np.float32),
                   np.zeros(600, np.float32)) as (dx, dw, dm, dv, dl, dlab, dpost, drow):
        for (n, d, k, niter, fl), code, word in (((8, 5, 257, 1, 0.1), "GR_ERR_UNSUPPORTED", "k 257"), ((8, 257, 2, 1, 0.1), "GR_ERR_UNSUPPORTED", "d 257"),
                                                 ((8, 5, 2, 1, 0.0), "GR_ERR_INVALID", "var_floor 0"), ((8, 5, 2, -1, 0.1), "GR_ERR_INVALID", "niter -1"),
                                                 ((0, 5, 2, 1, 0.1), "GR_ERR_INVALID", "n 0"), ((8, 5, 0, 1, 0.1), "GR_ERR_INVALID", "k 0"),
                                                 ((8, 5, 2, 1, float("nan")), "GR_ERR_INVALID", "var_floor")):
            with pytest.raises(L.GanrevError, match=code) as e:
                ctx.mixture_dev(dx, n, d, k, niter, fl, dw, dm, dv, dl, dlab, dpost, drow)
            assert word in str(e.value), str(e.value)
        for args in ((None, dw, dm, dv, dl), (dx, None, dm, dv, dl), (dx, dw, None, dv, dl), (dx, dw, dm, None, dl), (dx, dw, dm, dv, None)):
            with pytest.raises(L.GanrevError, match="GR_ERR_INVALID") as e:
                ctx.mixture_dev(args[0], 8, 5, 2, 1, 0.1, *args[1:])
            assert "null pointer" in str(e.value)
    m = mixture_dev(ctx, x, w, mu, var, 1, floor)                       # the context stays usable
    check_m_step((m["weights"], m["means"], m["variances"]), x, w, mu, var, floor, "after the refusals")


# ------------------------------------------------------------------ 5. member lists above 32 components
@pytest.mark.parametrize("k", [5, 33, 256])
def test_member_lists_are_a_stable_argsort(ctx, k):
    from ganrev import mixture as MX
    n, m = 3000, 9
    rng = np.random.default_rng(k)
    labels = rng.integers(0, k, n).astype(np.int32)
    post = rng.choice(np.linspace(0.5, 1.0, 40).astype(np.float32), n)      # many ties: the row decides
    lists = MX.members(ctx, labels, post, k, m)
    assert len(lists) == k
    for j in range(k):
        rows = np.nonzero(labels == j)[0]
        keep = rows[np.argsort(-post[rows], kind="stable")][:m]
        assert [r for r, _ in lists[j]] == keep.tolist(), j
        assert np.array_equal(bits(np.array([v for _, v in lists[j]], np.float32)), bits(post[keep])), j


# ------------------------------------------------------------------ 6. the script
BASE = ["--synthetic", "3x32x32x32", "--nbImages", "520", "--batchSize", "64", "--resident", "--render", "--nbClusters", "5", "--quiet"]
MIX_FILES = tuple("mixture_%s.npy" % q for q in ("weights", "means", "variances", "loglik", "labels", "posterior", "row_loglik"))


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
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("needle_faces")
    rng = np.random.default_rng(12)
    for i in range(3):
        np.save(d / ("face_%d.npy" % i), rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8))
    return str(d)


@pytest.fixture
def DATASET():
    from ganrev import dataset
    keys = ("dirs", "fileExtension", "height", "width", "nbChannels", "colorSpace", "paths", "_seed", "_draws")
    dataset.uncache()
    saved = {k: getattr(dataset, k) for k in keys}
    yield dataset
    dataset.uncache()
    for k, v in saved.items():
        setattr(dataset, k, v)


def check_run(ctx, tmp_path, options, d, space_file, needles=0):
    import ganrev._lib as L
    from ganrev import mixture as MX
    where, summary = run_apply_r(tmp_path, "mixture", "--mixture", "4", *options)
    plain, psummary = run_apply_r(tmp_path, "plain", *options)
    names = sorted(os.listdir(plain))
    assert "mixture" not in psummary and not [f for f in names if "mixture" in f]
    for f in names:                                                     # every file of the run without --mixture, byte for byte
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(where / f, "rb").read(), f
    timing = "embed_and_search_seconds"
    assert {q: v for q, v in summary.items() if q not in ("mixture", timing)} == {q: v for q, v in psummary.items() if q != timing}
    w, mu, var, ll, labels, post, rowll = (np.load(where / f) for f in MIX_FILES)
    assert (w.shape, mu.shape, var.shape, ll.shape, ll.dtype) == ((5,), (5, d), (5, d), (5,), np.float64)
    assert (labels.shape, labels.dtype, post.shape, rowll.shape) == ((520,), np.int32, (520,), (520,))
    entry = json.load(open(where / "summary.json"))["mixture"]
    assert entry == summary["mixture"] and entry["iterations"] == 4 and entry["k"] == 5 and entry["loglik"] == [float(v) for v in ll]
    assert entry["space"] == ("pca_whitened" if "--pcaSpace" in options else "attributes")
    # the files against the oracle, one iteration at a time from the parameters the library itself left: no error propagates
    table = np.load(where / space_file) if space_file else None
    if table is None:                                                   # --pcaSpace: the whitened projection, as apply_r computes it
        from ganrev import pca as P
        attrs = np.load(where / "attributes.npy")
        with on_device(ctx, attrs) as (da,):
            axes = P.principalAxes(ctx, da, 520, 32)
            try:
                t = P.project(ctx, axes, da, 520, d, whiten=True)
                table = t.numpy(); t.free()
            finally:
                axes.close()
    assert table.shape == (520, d)
    floor = np.float32(entry["var_floor"])
    w0, mu0, _ = mo.start(table, np.load(where / "cluster_centroids.npy"))
    step = dict(weights=w0, means=mu0)
    with on_device(ctx, table) as (dt,):
        pca_var = MX.columnVariances(ctx, dt, 520, d)                   # the initial variances are gr_pca_dev's covariance diagonal, as floats
    assert floor == np.float32(MX.VAR_FLOOR_FACTOR * pca_var.mean())    # the convention: 1e-3 x the mean column variance
    assert worst(np.abs(pca_var - table.astype(np.float64).var(axis=0, ddof=1)), np.diag(pp.cov_bound(table))) <= 1
    step["variances"] = np.tile(pca_var.astype(np.float32), (5, 1))
    for it in range(4):
        got = mixture_dev(ctx, table, step["weights"], step["means"], step["variances"], 1, floor)
        check_m_step((got["weights"], got["means"], got["variances"]), table, step["weights"], step["means"], step["variances"], floor, f"iteration {it}")
        assert got["loglik"][0] == ll[it]
        step = got
    assert np.array_equal(bits(step["weights"]), bits(w)) and np.array_equal(bits(step["means"]), bits(mu)) and np.array_equal(bits(step["variances"]), bits(var))
    assert step["loglik"][1] == ll[4]
    check_e_step(dict(rowll=rowll, labels=labels, post=post, loglik=float(ll[4])), table, w, mu, var, "the files' last E-step")
    # the pictures
    sizes = np.bincount(labels, minlength=5)
    for j in range(5):
        path = where / ("mixture_%02d.png" % (j + 1))
        assert os.path.exists(path) == bool(sizes[j])
        if sizes[j]:
            shown = 1 + min(int(sizes[j]), 71)
            _, gh, gw = L.grid_shape(shown, 1, 3, 32, 32, 0, int(np.ceil(np.sqrt(shown))))
            assert png_size(path) == (gw, gh), j
    _, gh, gw = L.grid_shape(520, 1, 3, 32, 32, 0, 22)
    assert png_size(where / "mixture_outliers.png") == (gw, gh)
    if needles:
        nm = np.load(where / "needle_mixture.npy")
        assert nm.shape == (needles, 3) and np.isfinite(nm).all() and ((nm[:, 0] >= 0) & (nm[:, 0] < 5)).all() and ((nm[:, 1] > 0) & (nm[:, 1] <= 1)).all()
        if space_file:                                                  # the needles' attribute rows under the files' mixture
            e = mo.e_step(np.load(where / "needle_attributes.npy"), w, mu, var)
            lb = mp.ell_bound(np.load(where / "needle_attributes.npy"), w, mu, var)
            assert worst(np.abs(nm[:, 2] - e["rowll"]), mp.rowll_bound(e, lb)) <= 1
    else:
        assert not os.path.exists(where / "needle_mixture.npy")
    return where


def test_apply_r_mixture(ctx, tmp_path):
    check_run(ctx, tmp_path, [], 32, "attributes.npy")


def test_apply_r_mixture_in_the_whitened_projection(ctx, tmp_path):
    check_run(ctx, tmp_path, ["--pca", "8", "--pcaSpace"], 8, None)


def test_apply_r_mixture_scores_the_needles(ctx, tmp_path, folder, DATASET):
    check_run(ctx, tmp_path, ["--needles", "2", "--dataset", folder, "--fileExtension", "npy"], 32, "attributes.npy", needles=2)
