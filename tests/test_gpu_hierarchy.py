"""gpu: gr_mst_dev (csrc/mst.hip) against the float64 oracle (tests/hierarchy_oracle.py) and the numpy restatement (tests/hierarchy_paths.py) - the
order of all pair distances of the test shapes is decided by the error bounds, so the edges must EQUAL the oracle's, in the same order, and the
weights agree within the bound; against the restatement every bit is equal - the cap on the rounds, the rules on integer data, long chains, the bit
identities with the pair chain and the neighbour graph, the DBSCAN identity of a cut, addressing, the refusals, ganrev.hierarchy and ganrev.apply_r
--hierarchy.  Outputs start from garbage (7)."""
import contextlib
import json
import math
import os

import numpy as np
import pytest

import density_paths as dp
import hierarchy_oracle as ho
import hierarchy_paths as hp
import silhouette_paths as sp
from test_hierarchy_host import (COLUMN_SHAPES, ROW_SHAPES, check_labels, check_planted, check_tree, planted, reference, reference_labels, samples_of,
                                 sizes_of)
from test_knn_host import same_bits, table

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


def round_cap(n):
    return max(1, math.ceil(math.log2(n)))


def mst_dev(ctx, x, metric, core=None, stride=1, misalign=False, n=None, d=None, null=None):
    """-> dict(u, v int32, w float64 [rows - 1], rounds); the outputs start at 7 and stay there where the call writes nothing.  core: a host array
    read with `stride` doubles from row to row (a column of a [rows x stride] table); n, d: the sizes passed, when they are not the table's"""
    x = np.ascontiguousarray(x, np.float32)
    rows, cols = x.shape
    n, d = rows if n is None else n, cols if d is None else d
    flat = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]) if misalign else x
    held = np.zeros(1) if core is None else np.ascontiguousarray(core, np.float64)
    with on_device(ctx, flat, held, np.full(rows - 1, 7, np.int32), np.full(rows - 1, 7, np.int32), np.full(rows - 1, 7.0)) as (dx, dk, du, dv, dw):
        args = dict(x=dx + 4 if misalign else dx, core=None if core is None else dk, u=du, v=dv, w=dw)
        if null:
            args[null] = None
        rounds = None
        try:
            rounds = ctx.mst_dev(args["x"], n, d, metric, args["core"], stride, args["u"], args["v"], args["w"])
        finally:
            got = dict(u=ctx.download(du, (rows - 1,), np.int32), v=ctx.download(dv, (rows - 1,), np.int32), w=ctx.download(dw, (rows - 1,), np.float64))
            mst_dev.last = got
        return dict(got, rounds=rounds)


def untouched(got):
    return all((np.asarray(got[q]) == 7).all() for q in ("u", "v", "w"))


def same_tree(a, b):
    return same_bits(np.asarray(a["u"], np.int32), np.asarray(b["u"], np.int32)) and same_bits(np.asarray(a["v"], np.int32), np.asarray(b["v"], np.int32)) \
        and same_bits(np.asarray(a["w"], np.float64), np.asarray(b["w"], np.float64))


def tree_of(t):
    return dict(u=t.u, v=t.v, w=t.w)


# ------------------------------------------------------------------ 1. against the oracle and the restatement
@pytest.mark.parametrize("metric", ho.METRICS)
@pytest.mark.parametrize("n,d", ROW_SHAPES + COLUMN_SHAPES)
def test_against_the_oracle(ctx, n, d, metric):
    from ganrev import hierarchy as HR
    x = reference(n, d, metric)[0]
    for s in samples_of(n):
        name = f"({n}, {d}) {metric} S {s}"
        t = HR.mst(ctx, x, s, metric)
        got = tree_of(t)
        r = check_tree(got, n, d, metric, s, name)                       # the oracle's edges, in its order; w within the bound
        again = hp.tree(x, s, metric)
        assert same_tree(got, again), name                               # the restatement's bits
        assert (t.core is None) == (s == 1) and (s == 1 or same_bits(t.core, again["core"])), name
        assert (t.u < t.v).all() and 1 <= t.rounds <= round_cap(n) and (t.n, t.minSamples, t.metric) == (n, s, metric), name
        print(f"{name}: {t.rounds} rounds (cap {round_cap(n)}), w err / bound {r:.3g}: equal")
        if d == 1 and metric == "cosine":
            continue
        for m in sizes_of(n):
            ref = reference_labels(n, d, metric, s, m)
            found = HR.hdbscan(t, m)
            check_labels(dict(labels=found.labels, prob=found.prob, clusters=found.clusters), ref, hp.prob_bound(ref, d, metric), f"{name} M {m}")


# ------------------------------------------------------------------ 2. the rules on integer data
def line(t):
    """points t (3, 4): every distance is a multiple of 5, exact in any order"""
    return np.asarray(t, np.float32)[:, None] * np.array([[3, 4]], np.float32)


def test_duplicate_rows_give_the_star_on_row_zero(ctx):
    x = np.repeat(np.array([[3, 4, -2]], np.float32), 70, axis=0)
    for metric in ho.METRICS:
        got = mst_dev(ctx, x, metric)
        assert got["u"].tolist() == [0] * 69 and got["v"].tolist() == list(range(1, 70)), metric
        assert same_bits(got["w"], np.zeros(69)) and got["rounds"] == 1, metric            # +0.0, not -0.0


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_collinear_points_with_equal_gaps_follow_the_order_rule(ctx, order):
    t = {"ascending": np.arange(40), "descending": np.arange(39, -1, -1), "shuffled": np.random.default_rng(8).permutation(40)}[order]
    x = line(t)
    at = np.argsort(t)                                                   # the row at every place of the line
    edges = sorted((int(min(a, b)), int(max(a, b))) for a, b in zip(at[:-1], at[1:]))
    got = mst_dev(ctx, x, "euclidean")
    assert list(zip(got["u"].tolist(), got["v"].tolist())) == edges and (got["w"] == 5.0).all() and got["rounds"] <= round_cap(40)
    for s in (2, 3, 5):                                                  # core distances that are multiples of 5: ties between edges that share no row
        core = hp.core_distances(x, s, "euclidean")
        got = mst_dev(ctx, x, "euclidean", core)
        assert same_tree(got, hp.tree(x, s, "euclidean")), (order, s)
        ref = ho.tree(x, s, "euclidean")
        assert np.array_equal(got["u"], ref["u"]) and np.array_equal(got["v"], ref["v"]) and np.array_equal(got["w"], ref["w"])       # integers: exact


def test_a_zero_row_under_cosine_is_at_distance_one_of_every_row(ctx):
    x = np.array([[1, 0], [2, 0], [0, 0], [0, 3], [-1, 0]], np.float32)
    got = mst_dev(ctx, x, "cosine")
    assert list(zip(got["u"].tolist(), got["v"].tolist(), got["w"].tolist())) == [(0, 1, 0.0), (0, 2, 1.0), (0, 3, 1.0), (2, 4, 1.0)]
    assert same_tree(got, hp.tree(x, 1, "cosine"))


def test_two_distant_clumps_are_joined_by_exactly_one_long_edge(ctx):
    grid = np.array([(a, b) for a in range(6) for b in range(6)], np.float32)
    x = np.concatenate([grid, grid + np.array([1000, 0], np.float32)])[np.random.default_rng(2).permutation(72)]
    for s in (1, 4):
        core = hp.core_distances(x, s, "euclidean")
        got = mst_dev(ctx, x, "euclidean", core)
        assert (got["w"] > 2).sum() == 1 and got["w"][-1] == 995.0 and same_tree(got, hp.tree(x, s, "euclidean")), s


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_a_long_chain_gives_the_restatements_bits(ctx, order):
    t = np.arange(299, -1, -1) if order == "descending" else np.random.default_rng(3).permutation(300)
    x = line(t)
    for s in (1, 3):
        got = mst_dev(ctx, x, "euclidean", hp.core_distances(x, s, "euclidean"))
        assert same_tree(got, hp.tree(x, s, "euclidean")) and got["rounds"] <= round_cap(300), (order, s)


# ------------------------------------------------------------------ 3. bit identities
@pytest.mark.parametrize("metric", ho.METRICS)
def test_the_weights_are_the_shared_chains_distances_and_the_neighbour_graphs(ctx, metric):
    """without core distances w IS pair_distances[u, v]; with them, the max of that and gr_knn_dev's two k-distances; the core column read in place
    with stride k equals a contiguous copy of it"""
    from ganrev import knn
    x = table(130, 100)
    chain = sp.pair_distances(x, metric)
    got = mst_dev(ctx, x, metric)
    assert same_bits(got["w"], chain[got["u"], got["v"]])
    g = knn.graph(ctx, x, 9, metric)
    for k in (1, 4, 9):
        kd = np.ascontiguousarray(g.dist[:, k - 1])
        copied = mst_dev(ctx, x, metric, kd)
        assert same_bits(copied["w"], np.maximum(np.maximum(chain[copied["u"], copied["v"]], kd[copied["u"]]), kd[copied["v"]])), k
        in_place = mst_dev(ctx, x, metric, g.dist.reshape(-1)[k - 1:], stride=9)                  # pointer dist + k - 1, stride 9
        assert same_tree(copied, in_place), k
        if k == 9:
            from ganrev import hierarchy as HR
            assert same_tree(copied, tree_of(HR.mst(ctx, x, 10, metric)))


@pytest.mark.parametrize("metric", ho.METRICS)
def test_a_cut_is_dbscan_at_that_eps(ctx, metric):
    """cut(tree, eps) restricted to the core rows is gr_dbscan_dev's partition of them at (eps, minPts = minSamples) - both number by smallest core
    row, so the labels themselves are equal - and every other row is -1: at density_paths.eps_for's eps, and at an eps that IS a core distance"""
    from ganrev import density, hierarchy as HR
    for n, d in [(129, 3), (513, 3)]:
        x = table(n, d)
        for s in (2, 5, 10):
            t = HR.mst(ctx, x, s, metric)
            for eps in (dp.eps_for(x, s, 0.7, metric), float(np.sort(t.core)[n // 2]), float(t.core.max())):
                found = density.cluster(ctx, x, eps, s, metric)
                labels = HR.cut(t, eps)
                assert np.array_equal(found.core, t.core <= eps), (n, s, eps)
                assert np.array_equal(labels[found.core], found.labels[found.core]) and (labels[~found.core] == -1).all(), (n, s, eps)
        t = HR.mst(ctx, x, 1, metric)                                    # minPts 1: every row is core
        eps = dp.eps_for(x, 1, 0.5, metric)
        assert np.array_equal(HR.cut(t, eps), density.cluster(ctx, x, eps, 1, metric).labels)


# ------------------------------------------------------------------ 4. reproducibility and addressing
def test_two_runs_agree(ctx):
    x = table(513, 3)
    for metric in ho.METRICS:
        core = hp.core_distances(x, 5, metric)
        assert same_tree(mst_dev(ctx, x, metric, core), mst_dev(ctx, x, metric, core))


def test_table_pointer_offset_by_four_bytes(ctx):
    x = table(130, 100)
    for metric in ho.METRICS:
        assert same_tree(mst_dev(ctx, x, metric), mst_dev(ctx, x, metric, misalign=True))


def test_a_prefix_of_a_larger_table_is_the_tree_of_the_prefix_alone(ctx):
    x = table(513, 3)
    for metric in ho.METRICS:
        core = hp.core_distances(x[:130], 5, metric)
        whole = mst_dev(ctx, x, metric, np.concatenate([core, np.full(383, 1e300)]), n=130)
        alone = mst_dev(ctx, x[:130], metric, core)
        assert all(same_bits(whole[q][:129], alone[q]) for q in ("u", "v", "w"))
        assert all((whole[q][129:] == 7).all() for q in ("u", "v", "w"))                          # nothing is written past the edges asked for


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_outputs_alone_and_the_next_call_works(ctx):
    import ganrev._lib as L
    x = table(200, 5)
    core = hp.core_distances(x, 4, "euclidean")
    before = mst_dev(ctx, x, "euclidean", core)
    for bad, word in ((dict(n=1), "n 1"), (dict(n=0), "n 0"), (dict(n=262145), "262145"), (dict(d=257), "257"), (dict(d=0), "d 0"),
                      (dict(metric=2), "metric 2"), (dict(stride=0), "core_stride 0"), (dict(stride=-3), "core_stride -3"),
                      (dict(null="x"), "null"), (dict(null="u"), "null"), (dict(null="v"), "null"), (dict(null="w"), "null")):
        with pytest.raises(L.GanrevError, match=word):
            mst_dev(ctx, x, bad.get("metric", "euclidean"), core, bad.get("stride", 1), n=bad.get("n"), d=bad.get("d"), null=bad.get("null"))
        assert untouched(mst_dev.last), bad
    assert same_tree(before, mst_dev(ctx, x, "euclidean", core))
    assert same_tree(before, hp.tree(x, 4, "euclidean"))


# ------------------------------------------------------------------ 6. the module
def test_the_module_finds_the_planted_blobs_without_an_eps(ctx):
    from ganrev import hierarchy as HR
    from ganrev.nn_utils import DeviceTensor
    x, blob, inner = planted()
    with DeviceTensor(ctx, x.shape) as t:
        ctx.upload(np.ascontiguousarray(x), t.ptr)
        found = [HR.cluster(ctx, source, 5, 15, "euclidean") for source in (x, t, (t.ptr, len(x), 2))]
        part = HR.cluster(ctx, t, 5, 15, "euclidean", rows=100)
    for f in found:
        check_planted(f.labels, f.clusters, blob, inner)
        assert same_tree(tree_of(f.tree), tree_of(found[0].tree)) and same_bits(f.labels, found[0].labels) and same_bits(f.prob, found[0].prob)
        assert (f.n, f.minSamples, f.minClusterSize, f.metric) == (len(x), 5, 15, "euclidean") and f.sizes.sum() + f.noise == len(x)
    assert same_tree(tree_of(found[0].tree), hp.tree(x, 5, "euclidean"))
    assert part.n == 100 and same_tree(tree_of(part.tree), hp.tree(x[:100], 5, "euclidean"))
    Z = HR.linkage(found[0].tree)
    assert Z.shape == (len(x) - 1, 4) and same_bits(Z[:, 2], found[0].tree.w) and Z[-1, 3] == len(x)


# ------------------------------------------------------------------ 7. apply_r --hierarchy
BASE = ["--synthetic", "1x32x32x32", "--nbImages", "520", "--resident", "--quiet"]
NEW_FILES = ["hierarchy_core.npy", "hierarchy_labels.npy", "hierarchy_linkage.npy", "hierarchy_mst_u.npy", "hierarchy_mst_v.npy", "hierarchy_mst_w.npy",
             "hierarchy_prob.npy"]
SCORES = ["silhouette_hierarchy_cosine.npy", "silhouette_hierarchy_euclidean.npy"]


def check_run(ctx, where, summary, space, s, m, rows=520, metric="cosine", cut=None):
    """the files of a run against ganrev.hierarchy recomputed from `space`, the table the run clustered; the summary's counts"""
    from ganrev import hierarchy as HR
    entry = json.load(open(where / "summary.json"))["hierarchy"]
    assert entry == summary["hierarchy"]
    assert sorted(entry) == sorted(["clusters", "metric", "minClusterSize", "minSamples", "noise", "rounds", "rows", "sizes", "space", "weight_quartiles"]
                                   + (["cut"] if cut is not None else []))
    assert (entry["minSamples"], entry["minClusterSize"], entry["metric"], entry["rows"]) == (s, m, metric, rows)
    found = HR.cluster(ctx, space, s, m, metric, rows=rows)
    u, v, w, core, Z, labels, prob = (np.load(where / f"hierarchy_{q}.npy") for q in ("mst_u", "mst_v", "mst_w", "core", "linkage", "labels", "prob"))
    assert u.dtype == v.dtype == labels.dtype == np.int32 and w.dtype == core.dtype == prob.dtype == Z.dtype == np.float64
    assert same_tree(dict(u=u, v=v, w=w), tree_of(found.tree)) and same_bits(core, found.tree.core) and same_bits(Z, HR.linkage(found.tree))
    assert same_bits(labels, found.labels) and same_bits(prob, found.prob) and labels.shape == prob.shape == core.shape == (rows,)
    assert entry["clusters"] == found.clusters == labels.max() + 1 and entry["noise"] == int((labels < 0).sum()) and 1 <= entry["rounds"] <= round_cap(rows)
    assert entry["sizes"] == sorted(np.bincount(labels[labels >= 0], minlength=found.clusters).tolist(), reverse=True)[:20]
    assert entry["weight_quartiles"] == [float(q) for q in np.quantile(w, [0.0, 0.25, 0.5, 0.75, 1.0])]
    if cut is not None:
        at = np.load(where / "hierarchy_cut_labels.npy")
        assert at.dtype == np.int32 and np.array_equal(at, HR.cut(found.tree, cut))
        assert entry["cut"] == dict(height=cut, clusters=int(at.max()) + 1, noise=int((at < 0).sum()))
    return entry, labels


def test_apply_r_hierarchy(ctx, tmp_path):
    from ganrev import apply_r, silhouette
    alone, where, plain = tmp_path / "alone", tmp_path / "all", tmp_path / "plain"
    asummary = apply_r.main(BASE + ["--hierarchy", "--writeTo", str(alone)])
    options = ["--silhouette", "--density", "--densityMinPts", "4"]
    summary = apply_r.main(BASE + options + ["--hierarchy", "--hierarchyMinSamples", "2", "--hierarchyMinClusterSize", "5", "--hierarchyCut", "4e-8",
                                             "--render", "--writeTo", str(where)])
    psummary = apply_r.main(BASE + options + ["--writeTo", str(plain)])       # (without the pictures: they are not what changes)
    names = sorted(os.listdir(plain))
    assert "hierarchy" not in psummary and not [f for f in names if "hierarchy" in f]
    for f in names:                                                     # what a run without the options writes, the run with them writes too, byte for byte
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(where / f, "rb").read(), f
    timing = "embed_and_search_seconds"
    strip = lambda s: {q: ({a: b for a, b in v.items() if a != "hierarchy"} if q == "silhouette" else v) for q, v in s.items() if q not in ("hierarchy", timing)}
    assert strip(summary) == strip(psummary)
    extra = sorted(set(os.listdir(where)) - set(names))
    attributes = np.load(where / "attributes.npy")
    entry, labels = check_run(ctx, where, summary, attributes, 2, 5, cut=4e-8)       # (the synthetic R's attributes lie 1e-8 apart under cosine)
    assert entry["clusters"] >= 2                                       # (so that the silhouette has something to score)
    assert sorted(f for f in extra if not f.endswith(".png")) == sorted(NEW_FILES + SCORES + ["hierarchy_cut_labels.npy"])
    pictures = [f for f in extra if f.endswith(".png") and f.startswith("hierarchy_")]       # (the other pictures are --render's)
    assert ("hierarchy_noise.png" in pictures) == (entry["noise"] > 0) and len([f for f in pictures if f != "hierarchy_noise.png"]) == min(entry["clusters"], 20)
    scored = summary["silhouette"]["hierarchy"]
    if 1 <= entry["clusters"] <= 4096:
        for metric in ("euclidean", "cosine"):
            ref = silhouette.score(ctx, attributes, labels, entry["clusters"], metric)
            assert np.array_equal(np.load(where / f"silhouette_hierarchy_{metric}.npy"), ref.values) and scored[metric]["mean"] == ref.mean
    else:
        assert "skipped" in scored
    # --hierarchy alone: the defaults, the seven files and nothing else new
    assert sorted(f for f in os.listdir(alone) if "hierarchy" in f) == NEW_FILES and "silhouette" not in asummary
    check_run(ctx, alone, asummary, np.load(alone / "attributes.npy"), 10, 25)


def test_apply_r_hierarchy_in_the_whitened_projection(ctx, tmp_path):
    from ganrev import apply_r
    where = tmp_path / "white"
    summary = apply_r.main(BASE + ["--pca", "8", "--pcaSpace", "--hierarchy", "--hierarchyMinSamples", "4", "--hierarchyMinClusterSize", "10",
                                   "--writeTo", str(where)])
    assert summary["hierarchy"]["space"] == "pca_whitened"
    attributes = np.load(where / "attributes.npy")
    n, d = attributes.shape
    with on_device(ctx, attributes, np.load(where / "pca_mean.npy"), np.load(where / "pca_axes.npy"), np.load(where / "pca_eigenvalues.npy"),
                   np.zeros((n, 8), np.float32)) as (da, dm, dx, dl, dw):
        ctx.pca_project_dev(da, n, d, dm, dx, dl, 8, True, dw)
        white = ctx.download(dw, (n, 8), np.float32)
    check_run(ctx, where, summary, white, 4, 10)
