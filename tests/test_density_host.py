"""cpu: the float64 DBSCAN oracle's own rules (tests/density_oracle.py), the numpy restatement of gr_eps_graph_dev's and gr_dbscan_dev's operations
(tests/density_paths.py) against it on the shapes tests/test_gpu_density.py runs, the condition that those shapes leave no pair's bit undecided,
scikit-learn as a third witness where it is installed, and the bindings and options."""
import functools

import numpy as np
import pytest

import density_oracle as do
import density_paths as dp
from test_knn_host import table

# the shapes (n, d) of tests/test_gpu_density.py: the smallest at which each loop can go wrong - rows around the 64-row tile (one output word) and the
# 512-row block, columns around the 16-column stage and at the limit, and the smallest n whose rows hold more than 64 words: a second step of the
# wave's word loop
ROW_SHAPES = [(n, 3) for n in (2, 3, 63, 64, 65, 129, 513)]
COLUMN_SHAPES = [(130, d) for d in (1, 2, 15, 16, 17, 100, 255, 256)]
WORD_SHAPES = [(4097, 3)]
SHAPES = ROW_SHAPES + COLUMN_SHAPES + WORD_SHAPES
RULES = ((2, 0.5), (4, 0.7), (10, 0.8))     # (minPts, the quantile of the k-distances eps is placed at): sparse, mixed and dense neighbourhoods
DECIDED_BY = 1e3                            # every pair's |dist - eps| is at least this many bounds wide: no implementation's rounding reaches it


def rules_of(n):
    """the rules a shape runs: minPts is at most n; the large shape runs the mixed one alone (its reference is the slow one)"""
    rules = RULES[1:2] if n > 1024 else RULES
    return tuple(dict.fromkeys((min(m, n), q) for m, q in rules))


@functools.lru_cache(maxsize=None)
def reference(n, d, metric):
    """per rule of a shape, computed once and left unchanged: eps, the oracle's words, counts, labels, core flags and cluster count, the number of
    undecided pairs and the smallest |dist - eps| / bound; the oracle's distance matrix is not kept"""
    x = table(n, d)
    dist = do.distances(x, metric)
    found = {}
    for m, q in rules_of(n):
        eps = dp.eps_for(x, m, q, metric, dist)
        adj, count = do.neighbourhoods(dist, eps)
        labels, core, clusters = do.dbscan(adj, m)
        open_pairs, ratio = dp.undecided(dist, eps, d, metric)
        entry = dict(eps=eps, words=dp.pack(adj), count=count.astype(np.int32), labels=labels.astype(np.int32), core=core, clusters=clusters,
                     undecided=open_pairs, ratio=ratio, kdist=do.kdistances(dist, m - 1) if m >= 2 else None)
        for a in entry.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        found[(m, q)] = entry
    return x, found


def check(got, ref, name):
    """got: dict(words, count, labels, core, clusters) from the code under test against the oracle's entry: equal, bit for bit"""
    assert ref["undecided"] == 0, f"{name}: {ref['undecided']} pairs whose bit the bounds do not decide: choose another eps"
    assert np.array_equal(np.asarray(got["words"], np.uint64), ref["words"]), name
    assert np.array_equal(np.asarray(got["count"], np.int64), ref["count"]), name
    assert np.array_equal(np.asarray(got["core"]).astype(bool), ref["core"]), name
    assert np.array_equal(np.asarray(got["labels"], np.int64), ref["labels"]), name
    assert int(got["clusters"]) == ref["clusters"], name


def restated(x, eps, m, metric):
    g = dp.graph(x, eps, metric)
    labels, core, clusters = dp.labels(g["adj"], g["count"], m)
    return dict(words=g["words"], count=g["count"], labels=labels, core=core, clusters=clusters)


# ------------------------------------------------------------------ 1. the restatement against the oracle; no pair is undecided
@pytest.mark.parametrize("metric", do.METRICS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_restatement_equals_the_oracle(n, d, metric):
    x, found = reference(n, d, metric)
    for (m, q), ref in found.items():
        check(restated(x, ref["eps"], m, metric), ref, f"({n}, {d}) {metric} minPts {m} q {q}")


@pytest.mark.parametrize("metric", do.METRICS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_no_pair_of_these_cases_is_undecided(n, d, metric):
    """the number of undecided pairs a case may have is zero, asserted on the oracle alone: an implementation's failure cannot hide behind it"""
    _, found = reference(n, d, metric)
    for (m, q), ref in found.items():
        noise, border = int((ref["labels"] < 0).sum()), int(((ref["labels"] >= 0) & ~ref["core"]).sum())
        print(f"({n}, {d}) {metric} minPts {m} q {q}: eps {ref['eps']:.6g}, smallest gap / bound {ref['ratio']:.3g}; {ref['clusters']} clusters, "
              f"{int(ref['core'].sum())} core, {border} border, {noise} noise rows")
        assert ref["undecided"] == 0 and ref["ratio"] > DECIDED_BY


def test_the_cases_have_several_clusters_border_rows_and_noise():
    for n, d in [(65, 3), (513, 3), (130, 100), (4097, 3)]:
        for metric in do.METRICS:
            ref = reference(n, d, metric)[1][(4, 0.7)]
            assert ref["clusters"] >= 3 and (ref["labels"] < 0).any() and ((ref["labels"] >= 0) & ~ref["core"]).any() and not ref["core"].all()


@pytest.mark.parametrize("metric", do.METRICS)
def test_core_rows_are_the_rows_whose_k_distance_is_within_eps(metric):
    """the textbook reading of minPts: count_i >= minPts iff the (minPts - 1)-th nearest other row lies within eps"""
    for n, d in [(65, 3), (130, 17)]:
        for (m, q), ref in reference(n, d, metric)[1].items():
            assert np.array_equal(ref["core"], ref["kdist"] <= ref["eps"])


@pytest.mark.parametrize("metric", do.METRICS)
@pytest.mark.parametrize("n,d", [(63, 3), (129, 3), (513, 3), (130, 2), (130, 100)])
def test_the_oracle_is_scikit_learns_dbscan(n, d, metric):
    cluster = pytest.importorskip("sklearn.cluster")
    x, found = reference(n, d, metric)
    dist = do.distances(x, metric)
    for (m, q), ref in found.items():
        fit = cluster.DBSCAN(eps=ref["eps"], min_samples=m, metric="precomputed").fit(dist)
        core = np.zeros(n, bool)
        core[fit.core_sample_indices_] = True
        assert np.array_equal(fit.labels_, ref["labels"]) and np.array_equal(core, ref["core"])


# ------------------------------------------------------------------ 2. the rules on integer data, on the oracle and the restatement alike
def by_oracle(x, eps, m, metric):
    adj, count = do.neighbourhoods(do.distances(x, metric), eps)
    labels, core, clusters = do.dbscan(adj, m)
    return dict(words=dp.pack(adj), count=count, labels=labels, core=core, clusters=clusters)


def line(t):
    """points t (3, 4): every distance is a multiple of 5, exact in any order"""
    return np.asarray(t, np.float32)[:, None] * np.array([[3, 4]], np.float32)


AROUND = [(0, 1), (0, -1), (1, 0)]      # what makes a point with a neighbour on its left a core row at minPts 5


def between_two_clusters(first):
    """unit grid, eps 1, minPts 5: the row at (0, 0) has the core rows (-1, 0) and (1, 0) for neighbours and nothing else - a border row of both
    clusters; `first`: which of the two sides comes first in row order, and so carries the lower number.  Row 0 is the border row."""
    side = lambda s: [(s, 0)] + [(s + s * dx if dy == 0 else s, dy) for dx, dy in AROUND]
    rows = [(0, 0)] + side(first) + side(-first)
    return np.array(rows, np.float32)


# (name, x, eps, minPts, metric, labels, counts or None)
RULE_CASES = [
    ("equality counts", line([0, 1, 2, 3, 5]), 5.0, 2, "euclidean", [0, 0, 0, 0, -1], [2, 3, 3, 2, 1]),
    ("a border row between two clusters, the left one first", between_two_clusters(-1), 1.0, 5, "euclidean", [0, 0, 0, 0, 0, 1, 1, 1, 1], [3, 5, 2, 2, 2, 5, 2, 2, 2]),
    ("a border row between two clusters, the right one first", between_two_clusters(1), 1.0, 5, "euclidean", [0, 0, 0, 0, 0, 1, 1, 1, 1], [3, 5, 2, 2, 2, 5, 2, 2, 2]),
    ("minPts 1: every row is core", line([0, 1, 5, 9, 10]), 5.0, 1, "euclidean", [0, 0, 1, 2, 2], [2, 2, 1, 2, 2]),
    ("no core row", line([0, 2, 4, 6]), 5.0, 2, "euclidean", [-1, -1, -1, -1], [1, 1, 1, 1]),
    ("duplicates at eps 0, euclidean", np.repeat(np.array([[3, 4, -2]], np.float32), 70, axis=0), 0.0, 70, "euclidean", [0] * 70, [70] * 70),
    ("duplicates at eps 0, cosine", np.repeat(np.array([[3, 4]], np.float32), 5, axis=0), 0.0, 5, "cosine", [0] * 5, [5] * 5),
    ("a zero row under cosine, out of reach", np.array([[1, 0], [2, 0], [0, 0], [0, 3], [-1, 0]], np.float32), 0.5, 2, "cosine", [0, 0, -1, -1, -1], [2, 2, 1, 1, 1]),
    ("a zero row under cosine, at distance exactly 1", np.array([[1, 0], [2, 0], [0, 0], [0, 3], [-1, 0]], np.float32), 1.0, 2, "cosine", [0] * 5, [4, 4, 5, 5, 3]),
]


@pytest.mark.parametrize("impl", [by_oracle, restated], ids=["oracle", "restated"])
@pytest.mark.parametrize("case", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_the_rules_on_integer_data(impl, case):
    _, x, eps, m, metric, labels, count = case
    got = impl(x, eps, m, metric)
    assert np.asarray(got["labels"]).tolist() == labels and np.asarray(got["count"]).tolist() == count
    assert got["clusters"] == max(labels) + 1 and np.array_equal(np.asarray(got["core"]), np.asarray(count) >= m)


def test_packing_puts_row_j_at_bit_j_mod_64_of_word_j_div_64():
    adj = np.zeros((2, 130), bool)
    adj[0, [0, 63, 64, 129]] = True
    adj[1, 65] = True
    words = dp.pack(adj)
    assert words.shape == (2, 3) and words.dtype == np.uint64
    assert words[0].tolist() == [1 | 1 << 63, 1, 2] and words[1].tolist() == [0, 2, 0]
    back, padding = dp.unpack(words, 130)
    assert np.array_equal(back, adj) and padding.shape == (2, 62) and not padding.any()


# ------------------------------------------------------------------ 3. bindings and options
def test_the_library_exports_and_binds_both_calls():
    import ganrev._lib as L
    from ganrev import density
    for name, nargs in (("gr_eps_graph_dev", 8), ("gr_dbscan_dev", 8)):
        assert name in L.EXPORTED_SYMBOLS and len(L._SIGS[name][1]) == nargs
        assert getattr(L.load_library(), name)
    assert callable(L.Context.eps_graph_dev) and callable(L.Context.dbscan_dev)
    assert (density.MAX_ROWS, density.MAX_COLUMNS) == (L.Context.DBSCAN_MAX_N, L.Context.DBSCAN_MAX_D) == (262144, 256)
    assert L.Context.DBSCAN_METRICS == {"euclidean": 0, "cosine": 1} and L.Context.DBSCAN_MAX_N == L.Context.KNN_MAX_N
    assert [L.Context.eps_words(n) for n in (1, 64, 65, 4096, 4097)] == [1, 1, 2, 64, 65]
    assert all(callable(f) for f in (density.epsGraph, density.dbscan, density.cluster, density.epsFromNeighbours)) and density.DeviceEpsGraph
    assert "WAITS" in L.Context.dbscan_dev.__doc__ and "no host wait" in L.Context.eps_graph_dev.__doc__       # the one call of the family that waits says so


def test_the_module_checks_its_arguments_before_the_device_sees_them():
    import ganrev._lib as L
    from ganrev import density
    density.checkShape(2, 1); density.checkShape(262144, 256, 0.0, 262144, "euclidean"); density.checkShape(65, 3, 1.5, 65)
    for args, word in (((1, 3), "n 1"), ((262145, 3), "262145"), ((10, 257), "257"), ((10, 0), "d 0"), ((10, 3, -1.0), "eps -1"),
                       ((10, 3, float("nan")), "eps nan"), ((10, 3, float("inf")), "eps inf"), ((10, 3, 1.0, 0), "minPts 0"), ((10, 3, 1.0, 11), "minPts 11")):
        with pytest.raises(L.GanrevError, match=word):
            density.checkShape(*args)
    with pytest.raises(L.GanrevError, match="manhattan"):
        density.checkShape(10, 3, 1.0, 2, "manhattan")
    for m in (1, 130):
        with pytest.raises(L.GanrevError, match=f"minPts {m}"):
            density.epsFromNeighbours(None, np.zeros((200, 3), np.float32), m)       # refused before the context is touched
    g = density.EpsGraph(dp.pack(np.eye(5, dtype=bool)), np.ones(5, np.int32))
    with pytest.raises(L.GanrevError, match="minPts 6"):
        density.dbscan(None, g, 6)
    assert np.array_equal(g.dense(), np.eye(5, dtype=bool))


BASE = ["--synthetic", "1x32x32x32", "--nbImages", "600"]


def test_the_options_and_their_defaults():
    from ganrev import apply_r
    plain = apply_r.parse(BASE)
    assert apply_r.densityOptions(plain) is None
    assert not any(hasattr(plain, name) for name in ("density",) + apply_r.DENSITY_OPTIONS)      # absent unless given
    assert apply_r.densityOptions(apply_r.parse(BASE + ["--density"])) == (10, None, 0.75, 600, "cosine")
    assert apply_r.densityOptions(apply_r.parse(["--synthetic", "1x32x32x32", "--nbImages", "300000", "--density"])) == (10, None, 0.75, 100000, "cosine")
    given = BASE + ["--density", "--densityMinPts", "4", "--densityEps", "0.25", "--densityRows", "500", "--densityMetric", "euclidean"]
    assert apply_r.densityOptions(apply_r.parse(given)) == (4, 0.25, None, 500, "euclidean")
    assert apply_r.densityOptions(apply_r.parse(BASE + ["--density", "--densityQuantile", "0.5", "--densityMinPts", "129"])) == (129, None, 0.5, 600, "cosine")
    assert apply_r.densityOptions(apply_r.parse(BASE + ["--density", "--densityEps", "0", "--densityMinPts", "1"])) == (1, 0.0, None, 600, "cosine")
    assert callable(apply_r.afterClustering(type("S", (), dict(OPT=apply_r.parse(BASE + ["--density"])))))      # a step after the clustering
    assert apply_r.afterClustering(type("S", (), dict(OPT=plain))) is None


@pytest.mark.parametrize("extra,words", [
    (["--density", "--densityEps", "0.1", "--densityQuantile", "0.5"], ("--densityEps", "--densityQuantile")),
    (["--density", "--densityMinPts", "1"], ("--densityMinPts", "1", "--densityEps")),
    (["--density", "--densityMinPts", "130"], ("--densityMinPts", "130", "129")),
    (["--density", "--densityMinPts", "0", "--densityEps", "0.1"], ("--densityMinPts", "0")),
    (["--density", "--densityMinPts", "601", "--densityEps", "0.1"], ("--densityMinPts", "601", "600")),
    (["--density", "--host"], ("--density", "--host")),
    (["--density", "--densityRows", "262145", "--nbImages", "300000"], ("--densityRows", "262145")),
    (["--density", "--densityRows", "601"], ("--densityRows", "601")),
    (["--density", "--densityRows", "1"], ("--densityRows", "1")),
    (["--density", "--densityEps", "-0.5"], ("--densityEps", "-0.5")),
    (["--density", "--densityEps", "nan"], ("--densityEps", "nan")),
    (["--density", "--densityQuantile", "1.5"], ("--densityQuantile", "1.5")),
    (["--density", "--densityMetric", "manhattan"], ("--densityMetric", "manhattan")),
    (["--densityMinPts", "4"], ("--densityMinPts", "--density")),
    (["--densityEps", "0.1"], ("--densityEps", "--density")),
    (["--densityRows", "100"], ("--densityRows", "--density")),
])
def test_refusals_name_the_option_and_the_value(extra, words, capsys):
    from ganrev import apply_r
    with pytest.raises(SystemExit):
        apply_r.parse(BASE + extra)
    err = capsys.readouterr().err
    assert all(w in err for w in words), err
