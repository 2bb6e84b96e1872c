"""cpu: the float64 silhouette oracle's own rules (tests/silhouette_oracle.py), the numpy restatement of gr_silhouette_dev's operation chains
against it within the bounds derived from those chains (tests/silhouette_paths.py) on the shapes tests/test_gpu_silhouette.py runs, and the
bindings and options."""
import functools

import numpy as np
import pytest

import silhouette_oracle as so
import silhouette_paths as sp

# the shapes (n, d, k) of tests/test_gpu_silhouette.py: the smallest at which each loop can go wrong - rows around the 64-row tile and the 512-row
# block, columns around the 16-column stage and at the limit, clusters from one to the limit (most of them empty)
ROW_SHAPES = [(n, 3, 3) for n in (2, 63, 64, 65, 129, 513)]
COLUMN_SHAPES = [(130, d, 4) for d in (1, 31, 32, 33, 100, 255, 256)]
CLUSTER_SHAPES = [(200, 5, k) for k in (1, 2, 33, 4096)]
SHAPES = ROW_SHAPES + COLUMN_SHAPES + CLUSTER_SHAPES
# labellings whose clusters end at chosen places of the 64-entry tiles of the grouped order: exactly at tile edges; three inside one tile
EDGE_SIZES, INSIDE_SIZES = (64, 64, 72), (70, 5, 6, 7, 112)
S_BOUND_CAP = 1e-9          # every row's bound on s stays below this on the Gaussian cases: a float implementation (errors near 1e-7) cannot hide in it


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
    assert np.isfinite(err).all() and not np.isnan(bound).any()
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@functools.lru_cache(maxsize=None)
def case(n, d, k):
    """(x, labels) of a shape: Gaussian blobs, labelled by a k-way split that mostly follows them (a tenth of the rows sit in a wrong cluster, so
    that s takes both signs); up to 8 blobs however many clusters"""
    groups = min(k, 8)
    x, group = so.blobs(n, d, groups, seed=11 * n + d)
    rng = np.random.default_rng(n + d + k)
    labels = (group + groups * rng.integers(0, max(k // groups, 1), n)) % k
    wrong = rng.random(n) < 0.1
    labels = np.where(wrong, rng.integers(0, k, n), labels).astype(np.int32)
    x.setflags(write=False); labels.setflags(write=False)
    return x, labels


@functools.lru_cache(maxsize=None)
def sized_case(sizes):
    x, _ = so.blobs(sum(sizes), 7, len(sizes), seed=sum(sizes))
    labels = so.labels_of_sizes(sizes, seed=len(sizes))
    x.setflags(write=False); labels.setflags(write=False)
    return x, labels


@functools.lru_cache(maxsize=None)
def reference(key, metric):
    """the oracle's result and the bounds of a case, computed once: key = a shape (n, d, k) or ("sizes", sizes)"""
    x, labels = sized_case(key[1]) if key[0] == "sizes" else case(*key)
    k = len(key[1]) if key[0] == "sizes" else key[2]
    ref = so.silhouette(x, labels, k, metric)
    return x, labels, k, ref, sp.bounds(ref, labels, k, x.shape[1], metric)


def check(got, key, metric, name=None):
    """got: dict(values, a, b, nearest, cluster_mean, sizes, mean) from the code under test, against the oracle within the bounds -> the ratios"""
    x, labels, k, ref, bd = reference(key, metric)
    name = name or f"{key} {metric}"
    assert float(bd["values_one_sided"].max()) < S_BOUND_CAP, f"{name}: a row's bound on s is {bd['values_one_sided'].max():.3g}: choose another case"
    assert np.array_equal(np.asarray(got["sizes"]), ref["sizes"])
    assert int(bd["undecided"].sum()) == 0, f"{name}: {int(bd['undecided'].sum())} rows whose nearest cluster the bounds do not decide"
    assert np.array_equal(np.asarray(got["nearest"]), ref["nearest"])
    ratios = {q: worst(np.abs(np.asarray(got[q], np.float64) - ref[q]), bd[q]) for q in ("a", "b", "values", "cluster_mean", "mean")}
    print(f"{name}: err / bound " + ", ".join(f"{q} {v:.3g}" for q, v in ratios.items()) + f"; largest bound on s {bd['values_one_sided'].max():.3g}")
    assert max(ratios.values()) <= 1
    return ratios


# ------------------------------------------------------------------ 1. the restated chains against the oracle, within the derived bounds
@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_restated_chain_holds_the_bounds(n, d, k, metric):
    x, labels = case(n, d, k)
    check(sp.chain(x, labels, k, metric), (n, d, k), metric)


@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("sizes", [EDGE_SIZES, INSIDE_SIZES])
def test_restated_chain_on_the_tile_edge_labellings(sizes, metric):
    x, labels = sized_case(sizes)
    check(sp.chain(x, labels, len(sizes), metric), ("sizes", sizes), metric)


def test_the_cases_score_on_both_sides_of_zero():
    """the inputs are no degenerate clustering: good rows and misplaced rows"""
    _, _, _, ref, _ = reference((513, 3, 3), "euclidean")
    assert (ref["values"] > 0.3).sum() > 300 and (ref["values"] < 0).sum() > 10


# ------------------------------------------------------------------ 2. the rules, on the oracle and the restatement alike
RULE_X = np.array([[0, 0], [1, 0], [0, 1], [5, 5], [6, 5], [9, 9]], np.float32)


@pytest.mark.parametrize("impl", [so.silhouette, sp.chain], ids=["oracle", "chain"])
@pytest.mark.parametrize("metric", so.METRICS)
def test_singletons_outsiders_and_a_lone_cluster(impl, metric):
    got = impl(RULE_X, np.array([0, 0, 0, 1, 1, 2]), 4, metric)         # cluster 2 a singleton, cluster 3 empty
    assert got["values"][5] == 0 and got["a"][5] == 0 and got["nearest"][5] in (0, 1) and got["b"][5] > 0
    assert got["sizes"].tolist() == [3, 2, 1, 0] and got["cluster_mean"][3] == 0 and got["cluster_mean"][2] == 0
    got = impl(RULE_X, np.array([0, 0, -1, 1, 1, 4]), 4, metric)        # -1 and k = 4: no cluster, nobody's member
    assert got["sizes"].tolist() == [2, 2, 0, 0]
    for q in ("values", "a", "b"):
        assert got[q][2] == 0 and got[q][5] == 0
    assert got["nearest"][2] == -1 and got["nearest"][5] == -1
    assert got["mean"] == pytest.approx(got["values"].sum() / 6, rel=1e-15)     # rows without a cluster count as 0
    got = impl(RULE_X, np.zeros(6, np.int64), 1, metric)                # no other cluster: s = 0, nearest = -1, a still the own mean
    assert not got["values"].any() and (got["nearest"] == -1).all() and not got["b"].any() and (got["a"] > 0).all()


@pytest.mark.parametrize("impl", [so.silhouette, sp.chain], ids=["oracle", "chain"])
def test_a_zero_row_has_cosine_distance_one_to_every_row(impl):
    x = np.array([[0, 0], [1, 0], [2, 0], [0, 3]], np.float32)
    got = impl(x, np.array([0, 0, 1, 1]), 2, "cosine")
    assert got["a"][0] == 1.0 and got["b"][0] == 1.0 and got["values"][0] == 0.0 and got["nearest"][0] == 1
    assert got["a"][1] == 1.0 and got["b"][1] == 0.5                    # row 1: distance 1 to the zero row, 0 to (2, 0), 1 to (0, 3)


@pytest.mark.parametrize("impl", [so.silhouette, sp.chain], ids=["oracle", "chain"])
def test_duplicate_rows_have_a_zero_and_a_tie_goes_to_the_lower_cluster(impl):
    t = np.array([-10, -9, 0, 0, 9, 10], np.float32)
    x = t[:, None] * np.array([[3, 4]], np.float32)                     # every distance a multiple of 5: every sum is exact
    got = impl(x, np.array([2, 2, 1, 1, 0, 0]), 3, "euclidean")
    assert got["a"][2] == 0 and got["b"][2] == 47.5 and got["nearest"][2] == 0 and got["values"][2] == 1.0
    assert got["nearest"].tolist() == [1, 1, 0, 0, 1, 1]


# ------------------------------------------------------------------ 3. bindings and options
def test_the_library_exports_and_binds_the_silhouette():
    import ganrev._lib as L
    from ganrev import silhouette
    assert "gr_silhouette_dev" in L._SIGS and len(L._SIGS["gr_silhouette_dev"][1]) == 14
    assert callable(L.Context.silhouette_dev) and callable(silhouette.score) and silhouette.Silhouette
    assert silhouette.MAX_ROWS == L.Context.SILHOUETTE_MAX_N == 262144
    assert L.load_library().gr_silhouette_dev


def test_the_module_checks_its_arguments_before_the_device_sees_them():
    import ganrev._lib as L
    from ganrev import silhouette
    silhouette.checkShape(2, 1, 1, "euclidean"); silhouette.checkShape(262144, 256, 4096, "cosine")
    for args, word in (((1, 3, 3), "n 1"), ((262145, 3, 3), "262145"), ((10, 257, 3), "257"), ((10, 0, 3), "d 0"), ((10, 3, 4097), "4097"), ((10, 3, 0), "k 0")):
        with pytest.raises(L.GanrevError, match=word):
            silhouette.checkShape(*args)
    with pytest.raises(L.GanrevError, match="manhattan"):
        silhouette.checkShape(10, 3, 3, "manhattan")


BASE = ["--synthetic", "1x32x32x32", "--nbImages", "600"]


def test_the_options_and_their_defaults():
    from ganrev import apply_r
    assert apply_r.silhouetteOptions(apply_r.parse(BASE)) is None
    assert apply_r.silhouetteOptions(apply_r.parse(BASE + ["--silhouette"])) == (600, [])
    assert apply_r.silhouetteOptions(apply_r.parse(["--synthetic", "1x32x32x32", "--nbImages", "300000", "--silhouette"])) == (100000, [])
    assert apply_r.silhouetteOptions(apply_r.parse(BASE + ["--silhouette", "--silhouetteRows", "500", "--silhouetteSweep", "4,8,4096"])) == (500, [4, 8, 4096])
    assert apply_r.silhouetteOptions(apply_r.parse(BASE + ["--silhouetteSweep", "2"])) == (600, [2])      # the sweep alone scores too
    assert not hasattr(apply_r.parse(BASE), "silhouette")               # absent unless given: a run without them is the run it was


@pytest.mark.parametrize("extra,words", [
    (["--silhouette", "--silhouetteRows", "262145", "--nbImages", "300000"], ("--silhouetteRows", "262145")),
    (["--silhouette", "--silhouetteRows", "601"], ("--silhouetteRows", "601")),
    (["--silhouette", "--silhouetteRows", "1"], ("--silhouetteRows",)),
    (["--silhouetteRows", "100"], ("--silhouetteRows", "--silhouette")),
    (["--silhouetteSweep", "4,0"], ("--silhouetteSweep", "0")),
    (["--silhouetteSweep", "4,4097"], ("--silhouetteSweep", "4097")),
    (["--silhouetteSweep", "4,x"], ("--silhouetteSweep",)),
    (["--silhouette", "--host"], ("--silhouette", "--host")),
])
def test_refusals_name_the_option_and_the_value(extra, words, capsys):
    from ganrev import apply_r
    with pytest.raises(SystemExit):
        apply_r.parse(BASE + extra)
    err = capsys.readouterr().err
    assert all(w in err for w in words), err
