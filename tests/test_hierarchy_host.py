"""cpu: the float64 reference of the spanning tree and of HDBSCAN (tests/hierarchy_oracle.py) against scikit-learn and SciPy where they are
installed, the numpy restatement of gr_mst_dev's and gr_hdbscan_host's operations (tests/hierarchy_paths.py) against it on the shapes
tests/test_gpu_hierarchy.py runs, the conditions that make "equal" the right demand on those shapes - asserted on the oracle alone -,
gr_hdbscan_host from the loaded library bit for bit against the restatement, ganrev.hierarchy's host functions, the bindings and the options."""
import functools
import os

import numpy as np
import pytest

import hierarchy_oracle as ho
import hierarchy_paths as hp
import silhouette_oracle as so
from test_knn_host import same_bits, table

# the shapes (n, d) of tests/test_gpu_hierarchy.py: rows around the 64-row tile and the 512-row block (two tiles of edges for the ranking), columns
# around the 16-column stage and at the limit; minSamples from plain single linkage to ten, clipped to n
ROW_SHAPES = [(n, 3) for n in (2, 3, 63, 64, 65, 129, 513)]
COLUMN_SHAPES = [(130, d) for d in (1, 2, 15, 16, 17, 100, 255, 256)]
SHAPES = ROW_SHAPES + COLUMN_SHAPES
MIN_SAMPLES = (1, 2, 5, 10)
MIN_CLUSTER_SIZES = (5, 25)
DECIDED_BY = 100.0          # every gap between consecutive pair distances is at least this many bounds wide: no implementation's rounding reaches it


def samples_of(n):
    return tuple(dict.fromkeys(min(s, n) for s in MIN_SAMPLES))


def sizes_of(n):
    return tuple(dict.fromkeys(max(2, min(m, n)) for m in MIN_CLUSTER_SIZES))


def exact_tie_case(n, d, metric):
    """one column under the cosine distance: every distance is exactly 0 or 2 in every implementation - compared bit for bit instead"""
    return d == 1 and metric == "cosine"


def frozen(entry):
    for a in entry.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return entry


@functools.lru_cache(maxsize=None)
def reference(n, d, metric):
    """computed once and left unchanged: the table, the oracle's distance matrix, whether the order of its entries is decided, and per minSamples
    the oracle's tree"""
    x = table(n, d)
    dist = ho.distances(x, metric)
    dist.setflags(write=False)
    open_pairs, ratio = hp.order_decided(dist, d, metric)
    trees = {s: frozen(ho.tree(x, s, metric, dist)) for s in samples_of(n)}
    return x, dist, (open_pairs, ratio), trees


@functools.lru_cache(maxsize=None)
def reference_labels(n, d, metric, s, m):
    t = reference(n, d, metric)[3][s]
    return ho.hdbscan(t["u"], t["v"], t["w"], n, m)


def check_tree(got, n, d, metric, s, name):
    """got: dict(u, v, w) from the code under test against the oracle's tree: the edges EQUAL, in the same order, the weights within the bound"""
    _, _, (open_pairs, ratio), trees = reference(n, d, metric)
    ref = trees[s]
    if exact_tie_case(n, d, metric):
        assert same_bits(np.asarray(got["u"], np.int64), ref["u"]) and same_bits(np.asarray(got["v"], np.int64), ref["v"]), name
        assert same_bits(np.asarray(got["w"], np.float64), ref["w"]), name
        return 0.0
    assert open_pairs == 0, f"{name}: {open_pairs} pairs of distances whose order the bounds do not decide: choose another table"
    assert np.array_equal(np.asarray(got["u"], np.int64), ref["u"]) and np.array_equal(np.asarray(got["v"], np.int64), ref["v"]), name
    r = worst_ratio(np.abs(np.asarray(got["w"], np.float64) - ref["w"]), hp.distance_bound(ref["w"], d, metric))
    assert r <= 1, f"{name}: w err / bound {r:.3g}"
    return r


def worst_ratio(err, bound):
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def same_partition(a, b):
    a, b = np.asarray(a).tolist(), np.asarray(b).tolist()
    pairs = set(zip(a, b))
    return all((p < 0) == (q < 0) for p, q in pairs) and len(pairs) == len({p for p, _ in pairs}) == len({q for _, q in pairs})


def check_labels(got, ref, bound, name):
    """got: dict(labels, prob, clusters) against the oracle's: the labels equal (both number by smallest member row), prob within the bound"""
    assert np.array_equal(np.asarray(got["labels"], np.int64), ref["labels"]) and int(got["clusters"]) == ref["clusters"], name
    r = worst_ratio(np.abs(np.asarray(got["prob"]) - ref["prob"]), bound)
    assert r <= 1, f"{name}: prob err / bound {r:.3g}"
    return r


def by_library(u, v, w, n, m):
    import ganrev._lib as L
    labels, prob, clusters = L.hdbscan_host(u, v, w, n, m)
    return dict(labels=labels, prob=prob, clusters=clusters)


def library_equals_restatement(u, v, w, n, m, name=""):
    got, ref = by_library(u, v, w, n, m), hp.hdbscan(u, v, w, n, m)
    assert same_bits(got["labels"], ref["labels"]) and same_bits(got["prob"], ref["prob"]) and got["clusters"] == ref["clusters"], name
    return got


# ------------------------------------------------------------------ 1. the conditions, on the oracle alone
@pytest.mark.parametrize("metric", ho.METRICS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_the_order_of_all_pair_distances_is_decided(n, d, metric):
    """the number of undecided shapes is zero - but for one column under cosine, whose distances are exactly 0 or 2 everywhere"""
    _, dist, (open_pairs, ratio), _ = reference(n, d, metric)
    print(f"({n}, {d}) {metric}: {n * (n - 1) // 2} pair distances, smallest gap / bound {ratio:.3g}")
    if exact_tie_case(n, d, metric):
        assert set(np.unique(dist).tolist()) <= {0.0, 2.0}
        return
    assert open_pairs == 0 and ratio > DECIDED_BY


@pytest.mark.parametrize("metric", ho.METRICS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_every_excess_of_mass_comparison_is_decided(n, d, metric):
    """... by more than the bound on the two stability sums; the cap on undecided comparisons is zero.  The largest relative bound on prob is
    reported and capped: a float32 implementation (errors near 1e-7) cannot hide in it"""
    if exact_tie_case(n, d, metric):
        return                                                          # exact ties: compared bit for bit, no bound is needed
    seen = 0
    for s in samples_of(n):
        for m in sizes_of(n):
            ref = reference_labels(n, d, metric, s, m)
            open_, ratio = hp.selection_decided(ref, d, metric)
            bound = hp.prob_bound(ref, d, metric)
            print(f"({n}, {d}) {metric} S {s} M {m}: {ref['clusters']} clusters, {len(ref['compared'])} comparisons, smallest |S - own| / bound {ratio:.3g}, "
                  f"largest prob bound {bound.max():.3g}")
            assert open_ == 0 and bound.max() < 1e-9
            seen += len(ref["compared"])
    assert seen > 0 or n < 10


def test_the_cases_have_clusters_noise_and_comparisons_of_both_outcomes():
    took, kept, noisy = 0, 0, 0
    for n, d in [(129, 3), (513, 3), (130, 100)]:
        for metric in ho.METRICS:
            for s in (1, 5):
                ref = reference_labels(n, d, metric, s, 5)
                assert ref["clusters"] >= 2 and ((ref["prob"] > 0) & (ref["prob"] < 1)).any()
                took += sum(total > own for total, own, _ in ref["compared"]); kept += sum(not total > own for total, own, _ in ref["compared"])
                noisy += bool((ref["labels"] < 0).any())
    assert took > 0 and kept > 0 and noisy >= 3


# ------------------------------------------------------------------ 2. the restatement against the oracle
@pytest.mark.parametrize("metric", ho.METRICS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_restatement_equals_the_oracle(n, d, metric):
    x, _, _, trees = reference(n, d, metric)
    for s in samples_of(n):
        name = f"({n}, {d}) {metric} S {s}"
        got = hp.tree(x, s, metric)
        check_tree(got, n, d, metric, s, name)
        if s >= 2 and not exact_tie_case(n, d, metric):
            assert worst_ratio(np.abs(got["core"] - trees[s]["core"]), hp.distance_bound(trees[s]["core"], d, metric)) <= 1, name
        if exact_tie_case(n, d, metric):
            continue
        for m in sizes_of(n):
            ref = reference_labels(n, d, metric, s, m)
            check_labels(hp.hdbscan(got["u"], got["v"], got["w"], n, m), ref, hp.prob_bound(ref, d, metric), f"{name} M {m}")


def test_kruskal_under_a_strict_order_does_not_depend_on_how_ties_are_met():
    """all weights equal: the tree is the star on row 0 - the n - 1 smallest edges by (lo, hi) - whatever finds it"""
    u, v, w = ho.kruskal(np.ones((9, 9)))
    assert u.tolist() == [0] * 8 and v.tolist() == list(range(1, 9)) and (w == 1).all()


# ------------------------------------------------------------------ 3. scikit-learn and SciPy as third witnesses
def blob_table(n, d, seed):
    return so.blobs(n, d, 3, seed=seed)[0]


# (table, metric, minSamples): cases whose n - 1 oracle tree weights are pairwise distinct (asserted) - where weights tie, the merge order is each
# implementation's own.  Under the mutual-reachability distance ties are the rule (a row's core distance is the weight of several of its edges):
# the minSamples 5 and 10 cases were searched for
SKLEARN_CASES = [((65, 3), "euclidean", 2), ((65, 3), "euclidean", 10), ((65, 3), "cosine", 1), ((129, 3), "cosine", 2), ((513, 3), "euclidean", 1),
                 ((513, 3), "cosine", 2), ((130, 2), "cosine", 1), ((130, 100), "euclidean", 2), ((130, 256), "cosine", 1),
                 ((33, 3, 30), "euclidean", 5), ((33, 3, 30), "cosine", 5), ((33, 5, 3), "euclidean", 5)]


def witness_case(key, metric, s):
    x = table(*key) if len(key) == 2 else blob_table(*key)
    dist = ho.distances(x, metric)
    return x, dist, ho.tree(x, s, metric, dist)


@pytest.mark.parametrize("key,metric,s", SKLEARN_CASES, ids=[f"{k}-{m}-S{s}" for k, m, s in SKLEARN_CASES])
def test_the_oracle_is_scikit_learns_hdbscan(key, metric, s):
    cluster = pytest.importorskip("sklearn.cluster")
    if not hasattr(cluster, "HDBSCAN"):
        pytest.skip("this scikit-learn has no HDBSCAN")
    x, dist, t = witness_case(key, metric, s)
    n, d = x.shape
    assert len(np.unique(t["w"])) == n - 1, "the tree weights tie: not a witness case"
    assert hp.order_decided(dist, d, metric)[0] == 0
    for m in (5, 12):
        ref = ho.hdbscan(t["u"], t["v"], t["w"], n, m)
        fit = cluster.HDBSCAN(metric="precomputed", min_samples=s, min_cluster_size=m).fit(dist.copy())
        assert same_partition(fit.labels_, ref["labels"]), (key, metric, s, m)
        r = worst_ratio(np.abs(fit.probabilities_ - ref["prob"]), hp.prob_bound(ref, d, metric))
        print(f"{key} {metric} S {s} M {m}: {ref['clusters']} clusters, {(ref['labels'] < 0).sum()} noise rows, prob err / bound {r:.3g}")
        assert r <= 1
        library_equals_restatement(t["u"].astype(np.int32), t["v"].astype(np.int32), t["w"], n, m)
        check_labels(by_library(t["u"], t["v"], t["w"], n, m), ref, hp.prob_bound(ref, d, metric), str(key))


def test_six_witness_cases_and_min_samples_five_among_them():
    assert len(SKLEARN_CASES) >= 6 and any(s == 5 for _, _, s in SKLEARN_CASES)


@pytest.mark.parametrize("metric", ho.METRICS)
@pytest.mark.parametrize("n,d", [(65, 3), (513, 3), (130, 100)])
def test_the_oracles_tree_against_scipy(n, d, metric):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    distance = pytest.importorskip("scipy.spatial.distance")
    from ganrev import hierarchy as HR
    _, dist, _, trees = reference(n, d, metric)
    for s in samples_of(n):
        t = trees[s]
        w = ho.weights(dist, t["core"])
        total = csgraph.minimum_spanning_tree(np.triu(w, 1)).sum()
        assert abs(total - t["w"].sum()) <= 4 * n * np.finfo(np.float64).eps * total, (s, total, t["w"].sum())
        np.fill_diagonal(w, 0.0)
        Z = hierarchy.linkage(distance.squareform(w, checks=False), "single")
        mine = HR.linkage(HR.SpanningTree(t["u"].astype(np.int32), t["v"].astype(np.int32), t["w"]))
        assert np.array_equal(mine[:, 2], Z[:, 2]) and mine[-1, 3] == n                             # the heights (among equal ones SciPy merges in its own order)
        assert hierarchy.is_valid_linkage(mine) and hierarchy.is_monotonic(mine)
        flat = hierarchy.fcluster(mine, float(t["w"][n // 2]), "distance")                         # SciPy reads the matrix: the cut at a height, up to renaming
        assert same_partition(flat, HR.cut(HR.SpanningTree(t["u"].astype(np.int32), t["v"].astype(np.int32), t["w"]), float(t["w"][n // 2])))
        if len(np.unique(t["w"])) == n - 1:
            assert np.array_equal(mine, Z)                                                             # without ties, the merges themselves


# ------------------------------------------------------------------ 4. gr_hdbscan_host, bit for bit against the restatement
def random_tree(n, seed, weights="gaussian"):
    """a random spanning tree with eu < ev, its edges in ascending (w, lo, hi) order"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    a = order[1:]
    b = np.array([order[rng.integers(0, i + 1)] for i in range(n - 1)])                          # every row hangs under an earlier one
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    w = {"gaussian": lambda: np.abs(rng.normal(size=n - 1)) + 1e-3, "few": lambda: rng.integers(1, 4, n - 1).astype(np.float64),
         "zeros": lambda: np.where(rng.random(n - 1) < 0.4, 0.0, rng.integers(1, 3, n - 1).astype(np.float64)),
         "equal": lambda: np.full(n - 1, 2.5)}[weights]()
    at = np.lexsort((hi, lo, w))
    return lo[at].astype(np.int32), hi[at].astype(np.int32), w[at]


@pytest.mark.parametrize("weights", ["gaussian", "few", "zeros", "equal"])
def test_the_library_is_the_restatement_on_random_trees(weights):
    for n, seed in [(2, 1), (3, 2), (17, 3), (200, 4), (1000, 5)]:
        u, v, w = random_tree(n, seed, weights)
        for m in sorted({2, min(5, n), min(40, n), n}):
            got = library_equals_restatement(u, v, w, n, m, f"{weights} n {n} M {m}")
            assert got["labels"].max() + 1 == got["clusters"] and ((got["prob"] >= 0) & (got["prob"] <= 1)).all()
            assert ((got["labels"] < 0) == (got["prob"] == 0)).all() or weights == "zeros"       # (a finite lambda against an infinite one is 0 too)
            if m == n:
                assert got["clusters"] == 0 and (got["labels"] == -1).all()                           # the root is never selected


def test_the_library_is_the_restatement_on_the_test_shapes():
    for (n, d), metric in [((513, 3), "cosine"), ((130, 100), "euclidean"), ((130, 1), "cosine"), ((3, 3), "euclidean"), ((2, 3), "cosine")]:
        x = reference(n, d, metric)[0]
        for s in samples_of(n):
            t = hp.tree(x, s, metric)
            for m in sizes_of(n):
                library_equals_restatement(t["u"], t["v"], t["w"], n, m, f"({n}, {d}) {metric} S {s} M {m}")


def chain_tree(weights):
    n = len(weights) + 1
    return np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32), np.asarray(weights, np.float64)


def test_ties_and_zero_weights_follow_the_rules():
    # two runs of duplicates (w 0: lambda inf) a long way apart: two clusters, every row a full member
    u, v, w = chain_tree([0.0] * 9 + [0.0] * 9 + [7.0])
    u, v = np.array(list(range(9)) + list(range(10, 19)) + [9], np.int32), np.array(list(range(1, 10)) + list(range(11, 20)) + [10], np.int32)
    got = library_equals_restatement(u, v, w, 20, 5)
    assert got["labels"].tolist() == [0] * 10 + [1] * 10 and (got["prob"] == 1).all() and got["clusters"] == 2
    # all weights equal: every split sheds one row at the same lambda; nothing but the root is ever born
    u, v, w = chain_tree([3.0] * 30)
    got = library_equals_restatement(u, v, w, 31, 2)
    assert (got["labels"] == -1).all() and got["clusters"] == 0 and (got["prob"] == 0).all()
    # min_cluster_size 2: two tight pairs and a straggler
    u, v, w = np.array([0, 2, 1, 3], np.int32), np.array([1, 3, 2, 4], np.int32), np.array([1.0, 1.0, 4.0, 8.0])
    got = library_equals_restatement(u, v, w, 5, 2)
    assert got["labels"].tolist() == [0, 0, 1, 1, -1] and got["prob"].tolist() == [1, 1, 1, 1, 0]
    # min_cluster_size n: only the root holds n rows
    assert (library_equals_restatement(u, v, w, 5, 5)["labels"] == -1).all()


def planted(seed=5):
    """three blobs of different spread and uniform noise around them -> (x, the blob of every row, -1 for the noise; inner: the rows within one
    standard deviation of their blob's centre)"""
    rng = np.random.default_rng(seed)
    centres, spreads, counts = np.array([[0, 0], [12, 0], [0, 14]], np.float64), (0.3, 1.0, 2.0), (60, 80, 100)
    parts, blob, inner = [], [], []
    for b, (c, s, k) in enumerate(zip(centres, spreads, counts)):
        p = rng.normal(size=(k, 2)) * s
        parts.append(c + p); blob += [b] * k; inner += (np.sqrt((p * p).sum(axis=1)) < s).tolist()
    parts.append(rng.uniform(-8, 22, size=(40, 2))); blob += [-1] * 40; inner += [False] * 40
    order = rng.permutation(len(blob))
    return np.concatenate(parts)[order].astype(np.float32), np.array(blob)[order], np.array(inner)[order]


def check_planted(labels, clusters, blob, inner):
    """three clusters; the inner rows of a blob share one label, and the three labels differ"""
    assert clusters == 3
    found = [set(labels[inner & (blob == b)].tolist()) for b in range(3)]
    assert all(len(f) == 1 and -1 not in f for f in found) and len(set.union(*found)) == 3
    assert (labels[blob < 0] < 0).sum() >= 20                                                     # most of the uniform rows are noise


def test_planted_blobs_of_different_spread_are_found_without_an_eps():
    x, blob, inner = planted()
    t = hp.tree(x, 5, "euclidean")
    got = library_equals_restatement(t["u"], t["v"], t["w"], len(x), 15)
    check_planted(got["labels"], got["clusters"], blob, inner)
    ref = ho.tree(x, 5, "euclidean")
    assert np.array_equal(ho.hdbscan(ref["u"], ref["v"], ref["w"], len(x), 15)["labels"], got["labels"])


def test_every_refusal_leaves_the_outputs_alone_and_a_good_call_follows():
    import ctypes as C
    import ganrev._lib as L
    lib = L.load_library()
    u, v, w = random_tree(12, 7)
    good = hp.hdbscan(u, v, w, 12, 3)

    def call(u=u, v=v, w=w, n=12, m=3, null=None):
        labels, prob, clusters = np.full(12, 7, np.int32), np.full(12, 7.0), C.c_int32(7)
        ptrs = [L._ptr(np.ascontiguousarray(u, np.int32)), L._ptr(np.ascontiguousarray(v, np.int32)), L._ptr(np.ascontiguousarray(w, np.float64)),
                L._ptr(labels), L._ptr(prob), C.byref(clusters)]
        if null is not None:
            ptrs[null] = None
        status = lib.gr_hdbscan_host(ptrs[0], ptrs[1], ptrs[2], n, m, ptrs[3], ptrs[4], ptrs[5])
        return status, labels, prob, clusters.value

    def edit(a, at, value):
        a = np.array(a)
        a[at] = value
        return a

    cycle_u, cycle_v = edit(u, 11 - 1, u[0]), edit(v, 11 - 1, v[0])                                # the last edge repeats the first
    bad = [dict(null=q) for q in range(6)] + [dict(n=1), dict(n=0), dict(n=-4), dict(m=1), dict(m=13), dict(m=0), dict(u=edit(u, 3, -1)),
           dict(v=edit(v, 3, 12)), dict(u=v, v=u), dict(u=edit(u, 5, v[5])), dict(w=edit(w, 2, -1.0)), dict(w=edit(w, 2, np.nan)),
           dict(w=edit(w, 10, np.inf)), dict(w=w[::-1].copy()), dict(u=cycle_u, v=cycle_v)]
    for kw in bad:
        status, labels, prob, clusters = call(**kw)
        assert status == -1, kw                                                                   # GR_ERR_INVALID
        assert (labels == 7).all() and (prob == 7).all() and clusters == 7, kw
    status, labels, prob, clusters = call()
    assert status == 0 and same_bits(labels, good["labels"]) and same_bits(prob, good["prob"]) and clusters == good["clusters"]
    with pytest.raises(L.GanrevError, match="min_cluster_size 13"):
        L.hdbscan_host(u, v, w, 12, 13)
    with pytest.raises(L.GanrevError, match="n - 1 edges"):
        L.hdbscan_host(u[:-1], v, w, 12, 3)


# ------------------------------------------------------------------ 5. ganrev.hierarchy on the host
def brute_force_cut(w, core, height):
    """the components of the threshold graph w_ij <= height over the rows with core <= height, numbered by smallest member row; -1 elsewhere"""
    n = len(w)
    alive = np.ones(n, bool) if core is None else core <= height
    labels, made = np.full(n, -1, np.int32), 0
    for seed in range(n):
        if not alive[seed] or labels[seed] >= 0:
            continue
        labels[seed], stack = made, [seed]
        while stack:
            p = stack.pop()
            for q in np.nonzero((w[p] <= height) & alive & (labels < 0))[0].tolist():
                labels[q] = made
                stack.append(q)
        made += 1
    return labels


@pytest.mark.parametrize("metric", ho.METRICS)
@pytest.mark.parametrize("n,d", [(65, 3), (129, 3), (130, 17)])
def test_cut_is_the_threshold_graphs_components(n, d, metric):
    from ganrev import hierarchy as HR
    _, dist, _, trees = reference(n, d, metric)
    for s in samples_of(n):
        t = trees[s]
        w = ho.weights(dist, t["core"])
        np.fill_diagonal(w, np.inf)
        tree = HR.SpanningTree(t["u"].astype(np.int32), t["v"].astype(np.int32), t["w"], t["core"], minSamples=s)
        heights = [0.0, float(t["w"][0]), float(t["w"][n // 2]), float(np.nextafter(t["w"][n // 2], 0)), float(t["w"][-1]), float(t["w"][-1]) * 2]
        heights += [float(np.median(t["core"])), float(t["core"].min())] if s >= 2 else []
        for h in heights:
            got = HR.cut(tree, h)
            assert got.dtype == np.int32 and np.array_equal(got, brute_force_cut(w, t["core"], h)), (s, h)
        assert (HR.cut(tree, float(t["w"][-1])) == 0).all()                                        # at the top everything is one cluster


def test_the_module_checks_its_arguments_before_the_device_sees_them():
    import ganrev._lib as L
    from ganrev import hierarchy as HR
    HR.checkShape(2, 1); HR.checkShape(262144, 256, 129, "euclidean"); HR.checkShape(65, 3, 65); HR.checkMinClusterSize(10, 2); HR.checkMinClusterSize(10, 10)
    for args, word in (((1, 3), "n 1"), ((262145, 3), "262145"), ((10, 257), "257"), ((10, 0), "d 0"), ((10, 3, 0), "minSamples 0"),
                       ((10, 3, 11), "minSamples 11"), ((500, 3, 130), "minSamples 130")):
        with pytest.raises(L.GanrevError, match=word):
            HR.checkShape(*args)
    with pytest.raises(L.GanrevError, match="manhattan"):
        HR.checkShape(10, 3, 1, "manhattan")
    for call, word in ((lambda: HR.mst(None, np.zeros((200, 3), np.float32), rows=201), "rows 201"),
                       (lambda: HR.cluster(None, np.zeros((200, 3), np.float32), 5, 1), "minClusterSize 1"),
                       (lambda: HR.cluster(None, np.zeros((200, 3), np.float32), 5, 201), "minClusterSize 201"),
                       (lambda: HR.cluster(None, np.zeros((200, 3), np.float32), 0, 5), "minSamples 0")):
        with pytest.raises(L.GanrevError, match=word):
            call()                                                                                # refused before the context is touched
    u, v, w = random_tree(12, 7)
    tree = HR.SpanningTree(u, v, w)
    for m in (1, 13):
        with pytest.raises(L.GanrevError, match=f"minClusterSize {m}"):
            HR.hdbscan(tree, m)
    for h in (-1.0, float("nan"), float("inf")):
        with pytest.raises(L.GanrevError, match="height"):
            HR.cut(tree, h)
    found = HR.hdbscan(tree, 3)
    ref = hp.hdbscan(u, v, w, 12, 3)
    assert same_bits(found.labels, ref["labels"]) and same_bits(found.prob, ref["prob"]) and found.clusters == ref["clusters"]
    assert found.noise == int((ref["labels"] < 0).sum()) and found.sizes.sum() + found.noise == 12 and (found.n, found.minClusterSize) == (12, 3)
    with pytest.raises(L.GanrevError, match="cycle"):
        HR.linkage(HR.SpanningTree(np.array([0, 0, 1], np.int32), np.array([1, 2, 2], np.int32), np.ones(3)))


def test_the_library_exports_and_binds_both_calls():
    import ganrev._lib as L
    from ganrev import hierarchy as HR
    for name, nargs in (("gr_mst_dev", 11), ("gr_hdbscan_host", 8)):
        assert name in L.EXPORTED_SYMBOLS and len(L._SIGS[name][1]) == nargs
        assert getattr(L.load_library(), name)
    assert callable(L.Context.mst_dev) and callable(L.hdbscan_host)
    assert (HR.MAX_ROWS, HR.MAX_COLUMNS, HR.MAX_MINSAMPLES) == (L.Context.MST_MAX_N, L.Context.MST_MAX_D, L.Context.KNN_MAX_K + 1) == (262144, 256, 129)
    assert L.Context.MST_METRICS == {"euclidean": 0, "cosine": 1} and L.Context.MST_MAX_N == L.Context.KNN_MAX_N
    assert all(callable(f) for f in (HR.mst, HR.hdbscan, HR.cluster, HR.linkage, HR.cut)) and HR.SpanningTree and HR.Clustering
    assert "WAITS" in L.Context.mst_dev.__doc__ and "WAITS" in L.Context.dbscan_dev.__doc__       # the calls of the family that wait say so
    assert "no GPU" in L.hdbscan_host.__doc__
    header = open(os.path.join(os.path.dirname(L.__file__), "..", "..", "include", "ganrev.h")).read()
    assert "gr_mst_dev WAITS ON THE STREAM" in header


# ------------------------------------------------------------------ 6. the options of apply_r
BASE = ["--synthetic", "1x32x32x32", "--nbImages", "600"]


def test_the_options_and_their_defaults():
    from ganrev import apply_r
    plain = apply_r.parse(BASE)
    assert apply_r.hierarchyOptions(plain) is None
    assert not any(hasattr(plain, name) for name in ("hierarchy",) + apply_r.HIERARCHY_OPTIONS)      # absent unless given
    assert apply_r.hierarchyOptions(apply_r.parse(BASE + ["--hierarchy"])) == (10, 25, 600, "cosine", None)
    assert apply_r.hierarchyOptions(apply_r.parse(["--synthetic", "1x32x32x32", "--nbImages", "300000", "--hierarchy"])) == (10, 25, 100000, "cosine", None)
    given = BASE + ["--hierarchy", "--hierarchyMinSamples", "4", "--hierarchyMinClusterSize", "12", "--hierarchyRows", "500", "--hierarchyMetric", "euclidean",
                    "--hierarchyCut", "0.25"]
    assert apply_r.hierarchyOptions(apply_r.parse(given)) == (4, 12, 500, "euclidean", 0.25)
    assert apply_r.hierarchyOptions(apply_r.parse(BASE + ["--hierarchy", "--hierarchyMinSamples", "1", "--hierarchyMinClusterSize", "2"]))[:2] == (1, 2)
    assert apply_r.hierarchyOptions(apply_r.parse(BASE + ["--hierarchy", "--hierarchyMinSamples", "129", "--hierarchyCut", "0"]))[::4] == (129, 0.0)
    assert callable(apply_r.afterClustering(type("S", (), dict(OPT=apply_r.parse(BASE + ["--hierarchy"])))))      # a step after the clustering
    assert apply_r.afterClustering(type("S", (), dict(OPT=plain))) is None
    assert apply_r.densityOptions(apply_r.parse(BASE + ["--hierarchy"])) is None                   # and no other step's


@pytest.mark.parametrize("extra,words", [
    (["--hierarchy", "--host"], ("--hierarchy", "--host")),
    (["--hierarchy", "--hierarchyMinSamples", "0"], ("--hierarchyMinSamples", "0")),
    (["--hierarchy", "--hierarchyMinSamples", "130"], ("--hierarchyMinSamples", "130", "129")),
    (["--hierarchy", "--hierarchyMinSamples", "101", "--hierarchyRows", "100"], ("--hierarchyMinSamples", "101", "100")),
    (["--hierarchy", "--hierarchyMinClusterSize", "1"], ("--hierarchyMinClusterSize", "1")),
    (["--hierarchy", "--hierarchyMinClusterSize", "601"], ("--hierarchyMinClusterSize", "601", "600")),
    (["--hierarchy", "--hierarchyRows", "262145", "--nbImages", "300000"], ("--hierarchyRows", "262145")),
    (["--hierarchy", "--hierarchyRows", "601"], ("--hierarchyRows", "601")),
    (["--hierarchy", "--hierarchyRows", "1"], ("--hierarchyRows", "1")),
    (["--hierarchy", "--hierarchyCut", "-0.5"], ("--hierarchyCut", "-0.5")),
    (["--hierarchy", "--hierarchyCut", "nan"], ("--hierarchyCut", "nan")),
    (["--hierarchy", "--hierarchyMetric", "manhattan"], ("--hierarchyMetric", "manhattan")),
    (["--hierarchyMinSamples", "4"], ("--hierarchyMinSamples", "--hierarchy")),
    (["--hierarchyMinClusterSize", "4"], ("--hierarchyMinClusterSize", "--hierarchy")),
    (["--hierarchyRows", "100"], ("--hierarchyRows", "--hierarchy")),
    (["--hierarchyMetric", "cosine"], ("--hierarchyMetric", "--hierarchy")),
    (["--hierarchyCut", "0.1"], ("--hierarchyCut", "--hierarchy")),
])
def test_refusals_name_the_option_and_the_value(extra, words, capsys):
    from ganrev import apply_r
    with pytest.raises(SystemExit):
        apply_r.parse(BASE + extra)
    err = capsys.readouterr().err
    assert all(w in err for w in words), err
