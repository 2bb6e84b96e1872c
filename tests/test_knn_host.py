"""cpu: the float64 k-nearest-neighbour oracle's own rules (tests/knn_oracle.py), the numpy restatement of gr_knn_dev's, gr_lof_dev's and
gr_knn_overlap_dev's operation chains against it within the bounds derived from those chains (tests/knn_paths.py) on the shapes
tests/test_gpu_knn.py runs, the condition that those shapes leave no row's list undecided, and the bindings and options."""
import functools

import numpy as np
import pytest

import knn_oracle as ko
import knn_paths as kp
from test_silhouette_host import case, worst

# the shapes (n, d, k) of tests/test_gpu_knn.py: the smallest at which each loop can go wrong - rows around the 64-row tile and the 512-row block,
# columns around the 16-column stage and at the limit, list lengths from one to the limit, around the 8 entries an insertion reads at a time, and
# the list that holds every other row
ROW_SHAPES = [(n, 3, min(10, n - 1)) for n in (2, 3, 63, 64, 65, 129, 513)]
COLUMN_SHAPES = [(130, d, 10) for d in (1, 2, 15, 16, 17, 100, 255, 256)]
K_SHAPES = [(200, 5, k) for k in (1, 2, 20, 64, 128)] + [(65, 3, 64)]
SHAPES = ROW_SHAPES + COLUMN_SHAPES + K_SHAPES
LOF_BOUND_CAP = 1e-9        # every row's relative bound on lof stays below this on the Gaussian cases: a float implementation (errors near 1e-7) cannot hide in it


def exact_tie_case(n, d, k, metric):
    """one column under the cosine distance: every distance is exactly 0 or 2, every list is full of ties - compared bit for bit instead"""
    return d == 1 and metric == "cosine"


def table(n, d):
    """the Gaussian blobs of tests/test_silhouette_host.py's case(n, d, 3), without the labels"""
    return case(n, d, 3)[0]


@functools.lru_cache(maxsize=None)
def reference(n, d, k, metric):
    """the oracle's graph, its outlier factors, which rows the bounds decide and the bounds, computed once"""
    x = table(n, d)
    ref = ko.knn(x, k, metric)
    ref_lof, ref_lrd = ko.lof(ref["idx"], ref["dist"])
    rows, ratio = kp.decided(ref, d, metric)
    for a in list(ref.values()) + [ref_lof, ref_lrd, rows]:
        a.setflags(write=False)
    return x, ref, (ref_lof, ref_lrd), rows, ratio, kp.lof_bounds(ref, ref_lof, ref_lrd, d, metric)


def same_bits(a, b):
    a, b = np.atleast_1d(np.ascontiguousarray(a)), np.atleast_1d(np.ascontiguousarray(b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.astype(a.dtype).view(np.uint8))


def check_graph(got, key, metric):
    """got: dict(idx, dist) from the code under test, against the oracle: the distances within the bound at every place of every row, and the
    lists themselves wherever the bounds decide them - everywhere, on these shapes"""
    x, ref, _, rows, ratio, bd = reference(*key, metric)
    name = f"{key} {metric}"
    if exact_tie_case(*key, metric):
        assert same_bits(np.asarray(got["idx"], np.int64), ref["idx"]) and same_bits(np.asarray(got["dist"], np.float64), ref["dist"]), name
        print(f"{name}: exact ties: idx and dist are the oracle's bits")
        return 0.0
    r = worst(np.abs(np.asarray(got["dist"], np.float64) - ref["dist"]), bd["dist"])
    print(f"{name}: dist err / bound {r:.3g}; smallest gap / bound {ratio:.3g}")
    assert r <= 1
    assert int((~rows).sum()) == 0, f"{name}: {int((~rows).sum())} rows whose list the bounds do not decide: choose another case"
    assert np.array_equal(np.asarray(got["idx"], np.int64), ref["idx"]), name
    return r


def check_lof(got_lof, got_lrd, key, metric):
    """against the oracle's factors of the oracle's graph: only where no row is undecided - with another neighbour set it is another number"""
    x, ref, (ref_lof, ref_lrd), rows, _, bd = reference(*key, metric)
    name = f"{key} {metric}"
    assert rows.all() and not exact_tie_case(*key, metric)
    assert float(bd["lof_relative"].max()) < LOF_BOUND_CAP, f"{name}: a row's bound on lof is {bd['lof_relative'].max():.3g}: choose another case"
    r_lrd, r_lof = worst(np.abs(got_lrd - ref_lrd), bd["lrd"]), worst(np.abs(got_lof - ref_lof), bd["lof"])
    print(f"{name}: err / bound lrd {r_lrd:.3g}, lof {r_lof:.3g}; largest relative bound on lof {bd['lof_relative'].max():.3g}")
    assert max(r_lrd, r_lof) <= 1


def shuffled_graph(idx, seed=5):
    """a copy of a graph in which row i keeps its first i % (k + 1) entries and the others are replaced by rows that are not in the list, every
    row's entries then shuffled -> (the copy, the known overlap count)"""
    rng = np.random.default_rng(seed)
    idx = np.asarray(idx)
    n, k = idx.shape
    out, keep = idx.copy(), np.arange(n) % (k + 1)
    for i in range(n):
        absent = np.setdiff1d(np.arange(n + k), idx[i])                 # (rows >= n: no row of the table, so never in the other list)
        out[i, keep[i]:] = absent[-(k - keep[i]):] if keep[i] < k else []
        rng.shuffle(out[i])
    return out.astype(np.int32), keep.astype(np.int32)


# ------------------------------------------------------------------ 1. the restated chains against the oracle, within the derived bounds
@pytest.mark.parametrize("metric", ko.METRICS)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_restated_chain_holds_the_bounds(n, d, k, metric):
    got = kp.graph(table(n, d), k, metric)
    check_graph(got, (n, d, k), metric)
    if not exact_tie_case(n, d, k, metric):
        check_lof(*kp.lof(got["idx"], got["dist"]), (n, d, k), metric)
    other, known = shuffled_graph(got["idx"])
    count, mean = kp.overlap(got["idx"], other)
    ref_count, ref_mean = ko.overlap(got["idx"], other)
    assert np.array_equal(count, known) and np.array_equal(ref_count, known) and abs(mean - ref_mean) <= kp.overlap_mean_bound(n)


@pytest.mark.parametrize("metric", ko.METRICS)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_no_row_of_these_cases_is_undecided(n, d, k, metric):
    """the share of undecided rows a case may have is zero, asserted on the oracle alone: an implementation's failure cannot hide behind it"""
    _, ref, _, rows, ratio, _ = reference(n, d, k, metric)
    if exact_tie_case(n, d, k, metric):
        assert np.isin(ref["ahead"], (0.0, 2.0)).all() and not rows.all()       # nothing but ties: bit for bit against the oracle instead
        return
    print(f"({n}, {d}, {k}) {metric}: smallest gap / bound {ratio:.3g}")
    assert rows.all() and ratio > 1e3


# ------------------------------------------------------------------ 2. the rules, on the oracle and the restatement alike
GRAPHS = pytest.mark.parametrize("impl", [ko.knn, kp.graph], ids=["oracle", "chain"])
FACTORS = pytest.mark.parametrize("impl,scorer", [(ko.knn, ko.lof), (kp.graph, kp.lof)], ids=["oracle", "chain"])


@GRAPHS
@pytest.mark.parametrize("metric", ko.METRICS)
def test_duplicates_come_first_at_distance_zero_in_index_order(impl, metric):
    x = np.array([[3, 4], [6, -8], [-2, 0.5], [3, 4], [0, 4], [3, 4], [6, -8]], np.float32)      # (norms 5 and 10: the cosine of a row with its copy is exactly 1)
    got = impl(x, 3, metric)
    assert got["idx"][3].tolist()[:2] == [0, 5] and got["idx"][0].tolist()[:2] == [3, 5] and got["idx"][5].tolist()[:2] == [0, 3]
    assert not got["dist"][[0, 3, 5], :2].any() and (got["dist"][[0, 3, 5], 2] > 0).all()
    assert got["idx"][1][0] == 6 and got["idx"][6][0] == 1 and got["dist"][1][0] == 0
    assert all(i not in got["idx"][i] for i in range(len(x)))           # a row is never its own neighbour


@GRAPHS
def test_a_zero_row_has_cosine_distance_one_to_every_row(impl):
    x = np.array([[1, 0], [2, 0], [0, 0], [0, 3], [-1, 0]], np.float32)
    got = impl(x, 3, "cosine")
    assert got["idx"][2].tolist() == [0, 1, 3] and got["dist"][2].tolist() == [1.0, 1.0, 1.0]      # all tie at 1: the lowest rows, without itself
    assert got["idx"][0].tolist() == [1, 2, 3] and got["dist"][0].tolist() == [0.0, 1.0, 1.0]      # (2, 0) at 0; the zero row and (0, 3) tie at 1


@GRAPHS
def test_a_tie_for_the_last_place_goes_to_the_lower_row(impl):
    t = np.array([0, 1, -1, 2, -2, 3, -3], np.float32)
    x = t[:, None] * np.array([[3, 4]], np.float32)                     # every distance a multiple of 5
    got = impl(x, 3, "euclidean")
    assert got["idx"][0].tolist() == [1, 2, 3] and got["dist"][0].tolist() == [5.0, 5.0, 10.0]     # rows 3 and 4 tie at 10: row 3 is kept


@FACTORS
@pytest.mark.parametrize("metric", ko.METRICS)
def test_lof_of_exact_duplicates_is_finite_and_one(impl, scorer, metric):
    k = 4
    x = np.concatenate([np.repeat(np.array([[0.5, -1.25, 3.0]], np.float32), k + 1, axis=0), np.array([[9, 9, -9], [7, -8, 9], [-8, 7.5, 9], [1, 30, 2], [-20, 1, 1]], np.float32)])
    g = impl(x, k, metric)
    lof, lrd = scorer(g["idx"], g["dist"])
    assert np.isfinite(lof).all() and np.isfinite(lrd).all() and (lof[:k + 1] == 1.0).all() and (lrd[:k + 1] == 1.0 / 1e-10).all()


@pytest.mark.parametrize("impl", [ko.overlap, kp.overlap], ids=["oracle", "chain"])
def test_a_graph_overlaps_itself_completely(impl):
    idx = kp.graph(table(513, 3), 10, "euclidean")["idx"]
    count, mean = impl(idx, idx)
    assert (count == 10).all() and mean == 1.0
    count, mean = impl(idx, idx[:, ::-1])                               # the order inside a row does not matter
    assert (count == 10).all() and mean == 1.0


# ------------------------------------------------------------------ 3. bindings and options
def test_the_library_exports_and_binds_the_three_calls():
    import ganrev._lib as L
    from ganrev import knn
    for name, nargs in (("gr_knn_dev", 8), ("gr_lof_dev", 7), ("gr_knn_overlap_dev", 7)):
        assert name in L.EXPORTED_SYMBOLS and len(L._SIGS[name][1]) == nargs
        assert getattr(L.load_library(), name)
    assert callable(L.Context.knn_dev) and callable(L.Context.lof_dev) and callable(L.Context.knn_overlap_dev)
    assert callable(knn.graph) and callable(knn.lof) and callable(knn.overlap) and knn.Graph and knn.DeviceGraph
    assert (knn.MAX_ROWS, knn.MAX_COLUMNS, knn.MAX_K) == (L.Context.KNN_MAX_N, L.Context.KNN_MAX_D, L.Context.KNN_MAX_K) == (262144, 256, 128)
    assert L.Context.KNN_METRICS == {"euclidean": 0, "cosine": 1} and L.Context.KNN_MAX_N == L.Context.SILHOUETTE_MAX_N


def test_the_module_checks_its_arguments_before_the_device_sees_them():
    import ganrev._lib as L
    from ganrev import knn
    knn.checkShape(2, 1, 1, "euclidean"); knn.checkShape(262144, 256, 128, "cosine"); knn.checkShape(65, 3, 64)
    for args, word in (((1, 3, 1), "n 1"), ((262145, 3, 3), "262145"), ((10, 257, 3), "257"), ((10, 0, 3), "d 0"), ((300, 3, 129), "129"), ((10, 3, 0), "k 0"),
                       ((10, 3, 10), "k 10")):
        with pytest.raises(L.GanrevError, match=word):
            knn.checkShape(*args)
    with pytest.raises(L.GanrevError, match="manhattan"):
        knn.checkShape(10, 3, 3, "manhattan")
    a, b = knn.Graph(np.zeros((5, 2), np.int32), np.zeros((5, 2))), knn.Graph(np.zeros((5, 3), np.int32), np.zeros((5, 3)))
    with pytest.raises(L.GanrevError, match="5 x 2 and 5 x 3"):
        knn.overlap(None, a, b)                                         # refused before the context is touched


BASE = ["--synthetic", "1x32x32x32", "--nbImages", "600"]


def test_the_options_and_their_defaults():
    from ganrev import apply_r
    plain = apply_r.parse(BASE)
    assert apply_r.outlierOptions(plain) is None and apply_r.mapNeighbourOptions(plain) is None
    assert not any(hasattr(plain, name) for name in ("outliers", "outlierRows", "outlierMetric", "mapNeighbours"))      # absent unless given
    assert apply_r.outlierOptions(apply_r.parse(BASE + ["--outliers", "10"])) == (10, 600, "cosine")
    assert apply_r.outlierOptions(apply_r.parse(["--synthetic", "1x32x32x32", "--nbImages", "300000", "--outliers", "128"])) == (128, 100000, "cosine")
    assert apply_r.outlierOptions(apply_r.parse(BASE + ["--outliers", "20", "--outlierRows", "500", "--outlierMetric", "euclidean"])) == (20, 500, "euclidean")
    assert apply_r.outlierOptions(apply_r.parse(BASE + ["--outliers", "9", "--outlierRows", "10"])) == (9, 10, "cosine")
    mapped = apply_r.parse(BASE + ["--map", "--mapRows", "300", "--mapNeighbours", "10"])
    assert apply_r.mapNeighbourOptions(mapped) == (10, "cosine") and apply_r.outlierOptions(mapped) is None
    assert apply_r.mapNeighbourOptions(apply_r.parse(BASE + ["--map", "--mapNeighbours", "7", "--outlierMetric", "euclidean"])) == (7, "euclidean")
    assert callable(apply_r.afterClustering(type("S", (), dict(OPT=apply_r.parse(BASE + ["--outliers", "10"])))))      # a step after the clustering
    assert apply_r.afterClustering(type("S", (), dict(OPT=plain))) is None


@pytest.mark.parametrize("extra,words", [
    (["--outliers", "129"], ("--outliers", "129")),
    (["--outliers", "0"], ("--outliers", "0")),
    (["--outliers", "10", "--outlierRows", "10"], ("--outliers", "10", "9")),
    (["--outliers", "10", "--outlierRows", "262145", "--nbImages", "300000"], ("--outlierRows", "262145")),
    (["--outliers", "10", "--outlierRows", "601"], ("--outlierRows", "601")),
    (["--outliers", "1", "--outlierRows", "1"], ("--outlierRows",)),
    (["--outlierRows", "100"], ("--outlierRows", "--outliers")),
    (["--outlierMetric", "cosine"], ("--outlierMetric", "--outliers")),
    (["--outliers", "10", "--outlierMetric", "manhattan"], ("--outlierMetric", "manhattan")),
    (["--outliers", "10", "--host"], ("--outliers", "--host")),
    (["--mapNeighbours", "10"], ("--mapNeighbours", "--map")),
    (["--map", "--mapRows", "300", "--mapNeighbours", "129"], ("--mapNeighbours", "129")),
    (["--map", "--mapRows", "100", "--mapNeighbours", "100"], ("--mapNeighbours", "100", "99")),
    (["--map", "--mapNeighbours", "0"], ("--mapNeighbours", "0")),
])
def test_refusals_name_the_option_and_the_value(extra, words, capsys):
    from ganrev import apply_r
    with pytest.raises(SystemExit):
        apply_r.parse(BASE + extra)
    err = capsys.readouterr().err
    assert all(w in err for w in words), err
