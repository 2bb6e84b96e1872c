"""gpu: gr_eps_graph_dev and gr_dbscan_dev (csrc/density.hip) against the float64 oracle (tests/density_oracle.py) and the numpy restatement
(tests/density_paths.py) - no pair of the test shapes is left undecided by the error bounds, so words, counts, core flags, labels and cluster
counts must be equal - the rules on integer data, many rounds of the component search, the bit identities, the refusals, and ganrev.apply_r
--density.  Outputs start from garbage (7)."""
import contextlib
import json
import os

import numpy as np
import pytest

import density_oracle as do
import density_paths as dp
import silhouette_paths as sp
from test_density_host import COLUMN_SHAPES, ROW_SHAPES, RULE_CASES, WORD_SHAPES, by_oracle, check, line, reference, restated
from test_knn_host import table

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


def words_of(n):
    return (n + 63) // 64


def graph_dev(ctx, x, eps, metric, misalign=False, n=None, d=None):
    """-> dict(words [rows x words_of(n)] uint64, count [rows] int32); both start at 7 and stay there where the call writes nothing.  n, d: the
    sizes passed, when they are not the table's (a prefix of the rows; a refusal)"""
    x = np.ascontiguousarray(x, np.float32)
    rows, cols = x.shape
    n, d = rows if n is None else n, cols if d is None else d
    w = words_of(min(max(n, 1), rows))                                   # (a refused n: the outputs are never indexed)
    flat = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]) if misalign else x
    with on_device(ctx, flat, np.full((rows, w), 7, np.uint64), np.full(rows, 7, np.int32)) as (dx, da, dc):
        try:
            ctx.eps_graph_dev(dx + 4 if misalign else dx, n, d, eps, metric, da, dc)
        finally:
            got = dict(words=ctx.download(da, (rows, w), np.uint64), count=ctx.download(dc, (rows,), np.int32))
            graph_dev.last = got
        return got


def dbscan_dev(ctx, words, count, m, with_core=True, n=None):
    """-> dict(labels, core, clusters) of a host copy of a bitmap; the outputs start at 7"""
    rows = len(count)
    n = rows if n is None else n
    with on_device(ctx, np.asarray(words, np.uint64), np.asarray(count, np.int32), np.full(rows, 7, np.int32), np.full(rows, 7, np.int32),
                   np.full(1, 7, np.int32)) as (da, dc, dl, dk, dn):
        try:
            ctx.dbscan_dev(da, dc, n, m, dl, dk if with_core else None, dn)
        finally:
            got = dict(labels=ctx.download(dl, (rows,), np.int32), core=ctx.download(dk, (rows,), np.int32), clusters=int(ctx.download(dn, (1,), np.int32)[0]))
            dbscan_dev.last = got
        return got


def cluster_dev(ctx, x, eps, m, metric):
    g = graph_dev(ctx, x, eps, metric)
    return dict(g, **dbscan_dev(ctx, g["words"], g["count"], m))


def untouched(got):
    return all((np.asarray(v) == 7).all() for v in got.values())


# ------------------------------------------------------------------ 1. against the oracle and the restatement: equal
@pytest.mark.parametrize("metric", do.METRICS)
@pytest.mark.parametrize("n,d", ROW_SHAPES + COLUMN_SHAPES + WORD_SHAPES)
def test_against_the_oracle(ctx, n, d, metric):
    x, found = reference(n, d, metric)
    for (m, q), ref in found.items():
        name = f"({n}, {d}) {metric} minPts {m} q {q}"
        got = cluster_dev(ctx, x, ref["eps"], m, metric)
        check(got, ref, name)
        check(restated(x, ref["eps"], m, metric), ref, name)            # (so the device equals the restatement too)
        adj, padding = dp.unpack(got["words"], n)
        assert np.array_equal(adj, adj.T), name                         # symmetric bit for bit
        assert adj.diagonal().all() and not padding.any(), name         # a row is in its own neighbourhood; nothing at or past n
        assert set(np.unique(got["core"]).tolist()) <= {0, 1}
        print(f"{name}: eps {ref['eps']:.6g}, {got['clusters']} clusters, {int(got['core'].sum())} core rows, {int((got['labels'] < 0).sum())} noise rows: equal")


@pytest.mark.parametrize("case", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_the_rules_on_integer_data(ctx, case):
    _, x, eps, m, metric, labels, count = case
    got = cluster_dev(ctx, x, eps, m, metric)
    assert got["labels"].tolist() == labels and got["count"].tolist() == count and got["clusters"] == max(labels) + 1
    assert np.array_equal(got["core"].astype(bool), np.asarray(count) >= m)


# ------------------------------------------------------------------ 2. one bitmap, several minPts
@pytest.mark.parametrize("metric", do.METRICS)
@pytest.mark.parametrize("n,d", [(129, 3), (513, 3)])
def test_one_bitmap_serves_every_min_pts(ctx, n, d, metric):
    x, found = reference(n, d, metric)
    ref = found[(4, 0.7)]
    g = graph_dev(ctx, x, ref["eps"], metric)
    adj, _ = dp.unpack(ref["words"], n)
    seen = set()
    for m in (1, 2, 4, 10, n):
        got = dbscan_dev(ctx, g["words"], g["count"], m)
        labels, core, clusters = do.dbscan(adj, m)
        assert np.array_equal(got["labels"], labels) and np.array_equal(got["core"].astype(bool), core) and got["clusters"] == clusters, m
        again, _, _ = dp.labels(adj, ref["count"], m)
        assert np.array_equal(got["labels"], again), m
        seen.add(clusters)
    assert len(seen) >= 3 and not (dbscan_dev(ctx, g["words"], g["count"], 1)["labels"] < 0).any()     # minPts 1: every row is core, none is noise


def test_the_core_flags_are_optional(ctx):
    x, found = reference(129, 3, "cosine")
    ref = found[(4, 0.7)]
    got = dbscan_dev(ctx, ref["words"], ref["count"], 4, with_core=False)
    assert np.array_equal(got["labels"], ref["labels"]) and (got["core"] == 7).all() and got["clusters"] == ref["clusters"]


# ------------------------------------------------------------------ 3. many rounds
def chain_points(order, missing=None):
    t = np.array([v for v in order if v != missing], np.float32)
    return line(t)


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_a_long_chain_is_one_cluster_whatever_the_row_order(ctx, order, m):
    """300 collinear points a spacing of exactly eps apart: one component of diameter 299, the worst case for the number of rounds.  With one
    point removed the chain falls into two clusters (at minPts 3 the rows beside the hole are border rows)."""
    t = np.arange(299, -1, -1) if order == "descending" else np.random.default_rng(3).permutation(300)
    for missing, clusters in ((None, 1), (150, 2)):
        x = chain_points(t, missing)
        got = cluster_dev(ctx, x, 5.0, m, "euclidean")
        ref = by_oracle(x, 5.0, m, "euclidean")
        assert got["clusters"] == ref["clusters"] == clusters and np.array_equal(got["labels"], ref["labels"]), (order, m, missing)
        assert np.array_equal(got["core"].astype(bool), ref["core"]) and np.array_equal(got["count"], ref["count"])
        if missing is None:
            assert (got["labels"] == 0).all() if m == 2 else (got["labels"] >= 0).all()
        assert np.array_equal(got["labels"], dp.labels(dp.unpack(got["words"], len(x))[0], got["count"], m)[0])


# ------------------------------------------------------------------ 4. bit identities
def same(a, b):
    return np.array_equal(a["words"], b["words"]) and np.array_equal(a["count"], b["count"])


@pytest.mark.parametrize("metric", do.METRICS)
def test_core_rows_are_where_the_neighbour_graphs_distance_is_within_eps(ctx, metric):
    """the pair distances are gr_knn_dev's bits: count_i >= minPts exactly where column minPts - 2 of its dist is <= eps - also at an eps that IS
    one of those distances, where a single differing bit would show"""
    from ganrev import knn
    x = table(513, 3)
    g = knn.graph(ctx, x, 9, metric)
    for m in (2, 4, 10):
        kd = g.dist[:, m - 2]
        for eps in (float(np.quantile(kd, 0.75)), float(np.sort(kd)[300]), float(kd.min()), float(kd.max())):
            got = cluster_dev(ctx, x, eps, m, metric)
            assert np.array_equal(got["core"].astype(bool), kd <= eps), (m, eps)


@pytest.mark.parametrize("metric", do.METRICS)
def test_the_counts_are_the_shared_chains_distances_within_eps(ctx, metric):
    x = table(130, 100)
    chain = sp.pair_distances(x, metric)
    off = ~np.eye(130, dtype=bool)
    for eps in (float(np.median(chain[off])), float(chain[3, 77]), 0.0):
        got = graph_dev(ctx, x, eps, metric)
        assert np.array_equal(got["count"] - 1, ((chain <= eps) & off).sum(axis=1)), eps
        assert np.array_equal(dp.unpack(got["words"], 130)[0] & off, (chain <= eps) & off), eps


def test_two_runs_agree(ctx):
    x, found = reference(513, 3, "euclidean")
    for metric in do.METRICS:
        eps = reference(513, 3, metric)[1][(4, 0.7)]["eps"]
        a, b = cluster_dev(ctx, x, eps, 4, metric), cluster_dev(ctx, x, eps, 4, metric)
        assert same(a, b) and np.array_equal(a["labels"], b["labels"]) and a["clusters"] == b["clusters"]


def test_table_pointer_offset_by_four_bytes(ctx):
    x = table(130, 100)
    for metric in do.METRICS:
        eps = reference(130, 100, metric)[1][(4, 0.7)]["eps"]
        assert same(graph_dev(ctx, x, eps, metric), graph_dev(ctx, x, eps, metric, misalign=True))


def test_a_prefix_of_a_larger_table_is_the_graph_of_the_prefix_alone(ctx):
    x = table(513, 3)
    for metric in do.METRICS:
        eps = reference(513, 3, metric)[1][(4, 0.7)]["eps"]
        whole = graph_dev(ctx, x, eps, metric, n=130)                    # (rows of words_of(130) = 3 words, 513 of them allocated)
        alone = graph_dev(ctx, x[:130], eps, metric)
        flat = whole["words"].reshape(-1)
        assert np.array_equal(flat[:130 * 3].reshape(130, 3), alone["words"]) and np.array_equal(whole["count"][:130], alone["count"])
        assert (flat[130 * 3:] == 7).all() and (whole["count"][130:] == 7).all()          # nothing is written past the rows asked for


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_outputs_alone_and_the_next_call_works(ctx):
    import ganrev._lib as L
    x = table(200, 5)
    eps = 2.0
    before = cluster_dev(ctx, x, eps, 4, "euclidean")
    for bad, word in ((dict(n=262145), "262145"), (dict(d=257), "257"), (dict(metric=2), "metric 2"), (dict(eps=-1.0), "eps -1"),
                      (dict(eps=float("nan")), "eps nan"), (dict(eps=float("inf")), "eps inf"), (dict(n=1), "n 1"), (dict(n=0), "n 0"), (dict(d=0), "d 0")):
        with pytest.raises(L.GanrevError, match=word):
            graph_dev(ctx, x, bad.get("eps", eps), bad.get("metric", "euclidean"), n=bad.get("n"), d=bad.get("d"))
        assert untouched(graph_dev.last), bad
    for bad, word in ((dict(m=0), "min_pts 0"), (dict(m=201), "min_pts 201"), (dict(m=-3), "min_pts -3"), (dict(n=262145, m=4), "262145"), (dict(n=1, m=1), "n 1")):
        with pytest.raises(L.GanrevError, match=word):
            dbscan_dev(ctx, before["words"], before["count"], bad["m"], n=bad.get("n"))
        assert untouched(dbscan_dev.last), bad
    with on_device(ctx, before["words"], before["count"], np.full(200, 7, np.int32), np.full(1, 7, np.int32)) as (da, dc, dl, dn):
        for call in (lambda: ctx.dbscan_dev(None, dc, 200, 4, dl, None, dn), lambda: ctx.dbscan_dev(da, dc, 200, 4, None, None, dn),
                     lambda: ctx.dbscan_dev(da, dc, 200, 4, dl, None, None), lambda: ctx.eps_graph_dev(None, 200, 5, eps, 0, da, dc)):
            with pytest.raises(L.GanrevError, match="null"):
                call()
        assert (ctx.download(dl, (200,), np.int32) == 7).all() and ctx.download(dn, (1,), np.int32)[0] == 7
        assert np.array_equal(ctx.download(da, before["words"].shape, np.uint64), before["words"])
    after = cluster_dev(ctx, x, eps, 4, "euclidean")
    assert same(before, after) and np.array_equal(before["labels"], after["labels"])


# ------------------------------------------------------------------ 6. the module
def test_the_module_keeps_a_graph_on_the_device(ctx):
    from ganrev import density
    from ganrev.nn_utils import DeviceTensor
    x, found = reference(129, 3, "cosine")
    ref = found[(4, 0.7)]
    with DeviceTensor(ctx, x.shape) as t:
        ctx.upload(np.ascontiguousarray(x), t.ptr)
        for source in (x, t, (t.ptr, 129, 3)):
            with density.epsGraph(ctx, source, ref["eps"]) as g:
                host = g.numpy()
                assert np.array_equal(host.words, ref["words"]) and np.array_equal(host.count, ref["count"]) and (g.n, g.metric) == (129, "cosine")
                found4, found2 = density.dbscan(ctx, g, 4), density.dbscan(ctx, g, 2)
            assert np.array_equal(found4.labels, ref["labels"]) and np.array_equal(found4.core, ref["core"]) and found4.clusters == ref["clusters"]
            assert np.array_equal(found4.count, ref["count"]) and np.array_equal(found4.sizes, np.bincount(ref["labels"][ref["labels"] >= 0], minlength=ref["clusters"]))
            assert np.array_equal(found2.labels, do.dbscan(dp.unpack(ref["words"], 129)[0], 2)[0])
            assert np.array_equal(density.dbscan(ctx, host, 4).labels, ref["labels"])          # a host copy is uploaded for the call
            assert np.array_equal(host.dense(), dp.unpack(ref["words"], 129)[0])
        part = density.cluster(ctx, t, ref["eps"], 4, "cosine", rows=70)
    alone = cluster_dev(ctx, x[:70], ref["eps"], 4, "cosine")
    assert np.array_equal(part.labels, alone["labels"]) and part.n == 70 and part.noise + part.border + int(part.core.sum()) == 70


@pytest.mark.parametrize("metric", do.METRICS)
def test_eps_from_the_neighbour_graph_makes_that_share_of_the_rows_core(ctx, metric):
    from ganrev import density, knn
    x = table(513, 3)
    eps, kdist = density.epsFromNeighbours(ctx, x, 10, 0.75, metric)
    assert np.array_equal(kdist, knn.graph(ctx, x, 9, metric).dist[:, 8]) and eps == float(np.quantile(kdist, 0.75))
    found = density.cluster(ctx, x, eps, 10, metric)
    assert np.array_equal(found.core, kdist <= eps) and abs(int(found.core.sum()) - 0.75 * 513) <= 1
    eps70, kd70 = density.epsFromNeighbours(ctx, x, 2, 0.5, metric, rows=70)
    assert len(kd70) == 70 and np.array_equal(kd70, knn.graph(ctx, x[:70], 1, metric).dist[:, 0])


# ------------------------------------------------------------------ 7. apply_r --density
BASE = ["--synthetic", "1x32x32x32", "--nbImages", "520", "--resident", "--quiet"]
NEW_FILES = ["density_core.npy", "density_count.npy", "density_kdist.npy", "density_labels.npy"]
SCORES = ["silhouette_density_cosine.npy", "silhouette_density_euclidean.npy"]


def check_run(ctx, where, summary, space, rows=520, m=4, metric="cosine"):
    """the files of a run against ganrev.density recomputed from `space`, the table the run clustered; the summary's counts"""
    from ganrev import density
    entry = json.load(open(where / "summary.json"))["density"]
    assert entry == summary["density"]
    assert sorted(entry) == ["border", "clusters", "core", "eps", "metric", "minPts", "noise", "quantile", "rows", "sizes", "space"]
    assert (entry["minPts"], entry["metric"], entry["rows"], entry["quantile"]) == (m, metric, rows, 0.75)
    eps, kdist = density.epsFromNeighbours(ctx, space, m, 0.75, metric, rows=rows)
    found = density.cluster(ctx, space, eps, m, metric, rows=rows)
    labels, core, count = (np.load(where / f"density_{q}.npy") for q in ("labels", "core", "count"))
    assert labels.dtype == core.dtype == count.dtype == np.int32 and labels.shape == core.shape == count.shape == (rows,)
    assert entry["eps"] == eps and np.array_equal(np.load(where / "density_kdist.npy"), kdist)
    assert np.array_equal(labels, found.labels) and np.array_equal(core.astype(bool), found.core) and np.array_equal(count, found.count)
    assert entry["clusters"] == found.clusters == labels.max() + 1 and entry["core"] == int(core.sum()) == int((kdist <= eps).sum())
    assert entry["noise"] == int((labels < 0).sum()) and entry["core"] + entry["border"] + entry["noise"] == rows
    assert entry["sizes"] == sorted(np.bincount(labels[labels >= 0]).tolist(), reverse=True)[:20] and sum(entry["sizes"]) <= rows - entry["noise"]
    return entry, labels


def test_apply_r_density(ctx, tmp_path):
    from ganrev import apply_r, silhouette
    where, plain, again = tmp_path / "dense", tmp_path / "plain", tmp_path / "again"
    options = ["--silhouette"]
    summary = apply_r.main(BASE + options + ["--density", "--densityMinPts", "4", "--render", "--writeTo", str(where)])
    psummary = apply_r.main(BASE + options + ["--writeTo", str(plain)])       # (without the pictures: they are not what changes)
    qsummary = apply_r.main(BASE + options + ["--writeTo", str(again)])
    names = sorted(os.listdir(plain))
    assert "density" not in psummary and not [f for f in names if "density" in f] and names == sorted(os.listdir(again))
    timing = "embed_and_search_seconds"
    for f in names:                                                     # without the options a run writes the same bytes twice, and the run with them too
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(again / f, "rb").read() == open(where / f, "rb").read(), f
    assert {q: v for q, v in psummary.items() if q != timing} == {q: v for q, v in qsummary.items() if q != timing}
    strip = lambda s: {q: ({a: b for a, b in v.items() if a != "density"} if q == "silhouette" else v) for q, v in s.items() if q not in ("density", timing)}
    assert strip(summary) == strip(psummary)
    extra = sorted(set(os.listdir(where)) - set(names))
    assert sorted(f for f in extra if not f.endswith(".png")) == sorted(NEW_FILES + SCORES)
    entry, labels = check_run(ctx, where, summary, np.load(where / "attributes.npy"))
    pictures = [f for f in extra if f.endswith(".png") and f.startswith("density_")]       # (the other pictures are --render's)
    assert ("density_noise.png" in pictures) == (entry["noise"] > 0) and len([f for f in pictures if f != "density_noise.png"]) == min(entry["clusters"], 20)
    scored = summary["silhouette"]["density"]
    if 1 <= entry["clusters"] <= 4096:
        for metric in ("euclidean", "cosine"):
            ref = silhouette.score(ctx, np.load(where / "attributes.npy"), labels, entry["clusters"], metric)
            assert np.array_equal(np.load(where / f"silhouette_density_{metric}.npy"), ref.values) and scored[metric]["mean"] == ref.mean
    else:
        assert "skipped" in scored


def test_apply_r_density_in_the_whitened_projection(ctx, tmp_path):
    from ganrev import apply_r
    where = tmp_path / "white"
    summary = apply_r.main(BASE + ["--pca", "8", "--pcaSpace", "--silhouette", "--density", "--densityMinPts", "4", "--writeTo", str(where)])
    assert summary["density"]["space"] == "pca_whitened"
    attributes = np.load(where / "attributes.npy")
    n, d = attributes.shape
    with on_device(ctx, attributes, np.load(where / "pca_mean.npy"), np.load(where / "pca_axes.npy"), np.load(where / "pca_eigenvalues.npy"),
                   np.zeros((n, 8), np.float32)) as (da, dm, dx, dl, dw):
        ctx.pca_project_dev(da, n, d, dm, dx, dl, 8, True, dw)
        white = ctx.download(dw, (n, 8), np.float32)
    check_run(ctx, where, summary, white)
    assert "density" in summary["silhouette"]
