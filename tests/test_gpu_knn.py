"""gpu: gr_knn_dev, gr_lof_dev and gr_knn_overlap_dev (csrc/knn.hip) against float64 numpy (tests/knn_oracle.py) within the bounds tests/knn_paths.py
derives from the library's operation chains - every numeric check asserts max err / bound <= 1 and prints the ratio - the bits of the restated
chains, the tie rule, the bit identities, the refusals, and ganrev.apply_r --outliers / --mapNeighbours.  Outputs start from garbage (7)."""
import contextlib
import json
import os

import numpy as np
import pytest

import knn_oracle as ko
import knn_paths as kp
import silhouette_paths as sp
from test_silhouette_host import worst
from test_knn_host import COLUMN_SHAPES, K_SHAPES, ROW_SHAPES, check_graph, check_lof, exact_tie_case, reference, same_bits, shuffled_graph, table

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


def knn_dev(ctx, x, k, metric, misalign=False, n=None, d=None):
    """-> dict(idx [rows x k] int32, dist [rows x k]); both start at 7 and stay there where the call writes nothing.  n, d: the sizes passed, when
    they are not the table's (a prefix of the rows; a refusal)"""
    x = np.ascontiguousarray(x, np.float32)
    rows, cols = x.shape
    n, d = rows if n is None else n, cols if d is None else d
    flat = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]) if misalign else x
    kk = max(k, 1)
    with on_device(ctx, flat, np.full((rows, kk), 7, np.int32), np.full((rows, kk), 7.0)) as (dx, di, dd):
        try:
            ctx.knn_dev(dx + 4 if misalign else dx, n, d, k, metric, di, dd)
        finally:
            got = dict(idx=ctx.download(di, (rows, kk), np.int32), dist=ctx.download(dd, (rows, kk), np.float64))
            knn_dev.last = got
        return got


def lof_dev(ctx, idx, dist, with_lrd=True):
    n, k = idx.shape
    with on_device(ctx, np.asarray(idx, np.int32), np.asarray(dist, np.float64), np.full(n, 7.0), np.full(n, 7.0)) as (di, dd, dl, dr):
        ctx.lof_dev(di, dd, n, k, dl, dr if with_lrd else None)
        return ctx.download(dl, (n,), np.float64), ctx.download(dr, (n,), np.float64)


def overlap_dev(ctx, a, b):
    n, k = a.shape
    with on_device(ctx, np.asarray(a, np.int32), np.asarray(b, np.int32), np.full(n, 7, np.int32), np.full(1, 7.0)) as (da, db, dc, dm):
        ctx.knn_overlap_dev(da, db, n, k, dc, dm)
        return ctx.download(dc, (n,), np.int32), float(ctx.download(dm, (1,), np.float64)[0])


def same_graph(a, b):
    return same_bits(np.asarray(a["idx"], np.int32), np.asarray(b["idx"], np.int32)) and same_bits(a["dist"], b["dist"])


# ------------------------------------------------------------------ 1. gr_knn_dev against the oracle, within the bounds
@pytest.mark.parametrize("metric", ko.METRICS)
@pytest.mark.parametrize("n,d,k", ROW_SHAPES + COLUMN_SHAPES + K_SHAPES)
def test_against_the_oracle(ctx, n, d, k, metric):
    check_graph(knn_dev(ctx, table(n, d), k, metric), (n, d, k), metric)


# ------------------------------------------------------------------ 2. the restated chains give the device's bits
@pytest.mark.parametrize("metric", ko.METRICS)
@pytest.mark.parametrize("n,d,k", [(65, 3, 10), (130, 33, 10), (513, 3, 10), (130, 1, 10), (200, 5, 128)])
def test_the_restated_chains_give_the_devices_bits(ctx, n, d, k, metric):
    """the order of every chain - columns, the walk over j, the list, the blocks of the mean - is the one the header states: tests/knn_paths.py,
    which performs those operations in that order in numpy, agrees bit for bit on idx, dist, lrd, lof, count and the overlap's mean"""
    x = table(n, d)
    got, ref = knn_dev(ctx, x, k, metric), kp.graph(x, k, metric)
    assert same_graph(got, ref)
    (lof, lrd), (ref_lof, ref_lrd) = lof_dev(ctx, got["idx"], got["dist"]), kp.lof(ref["idx"], ref["dist"])
    assert same_bits(lof, ref_lof) and same_bits(lrd, ref_lrd)
    other, known = shuffled_graph(ref["idx"])
    (count, mean), (ref_count, ref_mean) = overlap_dev(ctx, got["idx"], other), kp.overlap(ref["idx"], other)
    assert np.array_equal(count, known) and np.array_equal(ref_count, known) and same_bits(np.float64(mean), np.float64(ref_mean))


# ------------------------------------------------------------------ 3. ties on integer data
def test_ties_across_the_last_place_and_a_tile_edge(ctx):
    """points t (3, 4): every distance is a multiple of 5, exact in any order, so idx and dist are float64 numpy's bits.  Row 0 sits at t = 0; the
    rows at t = +-1 .. are placed so that pairs of equal distance lie on both sides of row 64 (two tiles of the walk), and the k-th place is
    fought over by two rows at the same distance: the lower row must win"""
    t = np.zeros(140)
    t[1:] = np.arange(1, 140)
    t[60:70] = [3, -3, 2, -2, 1, -1, 1, 2, 3, -4]                       # rows 64 and 65 at distance 5 on both sides; rows 60 .. 69 tie among themselves, across the tile edge
    t[100], t[130] = -7, 7                                              # ... and with rows 7, 100, 130 further on
    x = (t[:, None] * np.array([[3, 4]])).astype(np.float32)
    for k in (1, 2, 3, 5, 9, 10):
        got, ref = knn_dev(ctx, x, k, "euclidean"), ko.knn(x, k, "euclidean")
        assert same_graph(got, dict(idx=ref["idx"].astype(np.int32), dist=ref["dist"])), k
        assert same_graph(got, kp.graph(x, k, "euclidean")), k
    got = knn_dev(ctx, x, 3, "euclidean")
    assert got["idx"][0].tolist() == [1, 64, 65] and got["dist"][0].tolist() == [5.0, 5.0, 5.0]      # row 66 is at 5 too: the lower rows win
    got = knn_dev(ctx, x, 5, "euclidean")
    assert got["idx"][0].tolist() == [1, 64, 65, 66, 2] and got["dist"][0].tolist() == [5.0, 5.0, 5.0, 5.0, 10.0]     # rows 2, 62, 63, 67 at 10: row 2


@pytest.mark.parametrize("k", [1, 128])
def test_a_table_in_descending_order_of_nearness(ctx, k):
    """every later row is nearer to row 0: its list is rewritten at the head on every entry"""
    n = 200
    t = np.concatenate([[0], np.arange(n - 1, 0, -1)]).astype(np.float32)
    x = t[:, None] * np.array([[3, 4]], np.float32)
    got, ref = knn_dev(ctx, x, k, "euclidean"), ko.knn(x, k, "euclidean")
    assert same_graph(got, dict(idx=ref["idx"].astype(np.int32), dist=ref["dist"]))
    assert got["idx"][0].tolist() == list(range(n - 1, n - 1 - k, -1)) and got["dist"][0].tolist() == [5.0 * (p + 1) for p in range(k)]


# ------------------------------------------------------------------ 4. bit identities
def test_two_runs_agree(ctx):
    x = table(513, 3)
    for metric in ko.METRICS:
        assert same_graph(knn_dev(ctx, x, 10, metric), knn_dev(ctx, x, 10, metric))


def test_table_pointer_offset_by_four_bytes(ctx):
    x = table(130, 100)
    for metric in ko.METRICS:
        assert same_graph(knn_dev(ctx, x, 10, metric), knn_dev(ctx, x, 10, metric, misalign=True))


def test_a_prefix_of_a_larger_table_is_the_graph_of_the_prefix_alone(ctx):
    x = table(513, 3)
    for metric in ko.METRICS:
        whole = knn_dev(ctx, x, 10, metric, n=130)
        alone = knn_dev(ctx, x[:130], 10, metric)
        assert same_graph(dict(idx=whole["idx"][:130], dist=whole["dist"][:130]), alone)
        assert (whole["idx"][130:] == 7).all() and (whole["dist"][130:] == 7).all()       # nothing is written past the rows asked for


@pytest.mark.parametrize("metric", ko.METRICS)
def test_the_distances_are_the_silhouettes_chain(ctx, metric):
    """dist[i][p] is, bit for bit, the distance gr_silhouette_dev's chain gives the pair (i, idx[i][p]): as tests/silhouette_paths.py restates it, and
    as the device computes it - a of row i in a cluster of the two rows alone is that one distance (added to +0.0, divided by 1)"""
    x = table(130, 100)
    got = knn_dev(ctx, x, 10, metric)
    chain = sp.pair_distances(x, metric)
    assert same_bits(got["dist"], np.take_along_axis(chain, got["idx"].astype(np.int64), axis=1))
    from ganrev import silhouette
    for i, p in ((0, 0), (64, 9), (129, 3)):
        j = int(got["idx"][i][p])
        labels = np.full(130, -1, np.int32)
        labels[[i, j]] = 0
        assert same_bits(silhouette.score(ctx, x, labels, 1, metric).a[i], got["dist"][i][p])


def test_refusals_leave_the_outputs_alone_and_the_next_call_works(ctx):
    import ganrev._lib as L
    x = table(200, 5)
    before = knn_dev(ctx, x, 20, "euclidean")
    for bad, word in ((dict(n=262145), "262145"), (dict(k=200), "k 200"), (dict(k=129), "129"), (dict(d=257), "257"), (dict(metric=2), "metric 2"),
                      (dict(k=0), "k 0"), (dict(n=1, k=1), "n 1")):
        with pytest.raises(L.GanrevError, match=word):
            knn_dev(ctx, x, bad.get("k", 20), bad.get("metric", "euclidean"), n=bad.get("n"), d=bad.get("d"))
        assert (knn_dev.last["idx"] == 7).all() and (knn_dev.last["dist"] == 7).all(), bad
    with on_device(ctx, before["idx"], before["dist"], np.full(200, 7.0), np.full(200, 7, np.int32), np.full(1, 7.0)) as (di, dd, dl, dc, dm):
        for call, word in ((lambda: ctx.lof_dev(di, dd, 200, 129, dl), "129"), (lambda: ctx.lof_dev(di, dd, 262145, 20, dl), "262145"),
                           (lambda: ctx.lof_dev(di, None, 200, 20, dl), "null"), (lambda: ctx.knn_overlap_dev(di, di, 200, 200, dc, dm), "k 200"),
                           (lambda: ctx.knn_overlap_dev(di, None, 200, 20, dc, dm), "null")):
            with pytest.raises(L.GanrevError, match=word):
                call()
        assert (ctx.download(dl, (200,), np.float64) == 7).all() and (ctx.download(dc, (200,), np.int32) == 7).all() and ctx.download(dm, (1,), np.float64)[0] == 7
    assert same_graph(before, knn_dev(ctx, x, 20, "euclidean"))


# ------------------------------------------------------------------ 5. gr_lof_dev and gr_knn_overlap_dev against the oracle
@pytest.mark.parametrize("metric", ko.METRICS)
@pytest.mark.parametrize("n,d,k", ROW_SHAPES + COLUMN_SHAPES + K_SHAPES)
def test_lof_and_overlap_against_the_oracle(ctx, n, d, k, metric):
    got = knn_dev(ctx, table(n, d), k, metric)
    if not exact_tie_case(n, d, k, metric):                             # (with other neighbours it is another number: only where the lists are decided)
        check_lof(*lof_dev(ctx, got["idx"], got["dist"]), (n, d, k), metric)
    _, ref, _, _, _, _ = reference(n, d, k, metric)
    other, known = shuffled_graph(ref["idx"])
    count, mean = overlap_dev(ctx, got["idx"], other)
    ref_count, ref_mean = ko.overlap(ref["idx"], other)
    assert np.array_equal(count, known) and np.array_equal(count, ref_count) and abs(mean - ref_mean) <= kp.overlap_mean_bound(n)


def test_lrd_left_out_leaves_lof_unchanged(ctx):
    got = knn_dev(ctx, table(129, 3), 10, "cosine")
    (lof, lrd), (alone, untouched) = lof_dev(ctx, got["idx"], got["dist"]), lof_dev(ctx, got["idx"], got["dist"], with_lrd=False)
    assert same_bits(lof, alone) and (untouched == 7).all() and not (lrd == 7).any()


@pytest.mark.parametrize("metric", ko.METRICS)
def test_a_planted_outlier_has_the_largest_lof(ctx, metric):
    x = np.array(table(513, 3))
    direction = np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    x[300] = (x.mean(axis=0) + 10 * x.std(axis=0).max() * direction).astype(np.float32)     # 10 sigma out, where no blob lies
    got = knn_dev(ctx, x, 10, metric)
    lof, _ = lof_dev(ctx, got["idx"], got["dist"])
    ref = ko.knn(x, 10, metric)
    ref_lof, ref_lrd = ko.lof(ref["idx"], ref["dist"])
    assert kp.decided(ref, 3, metric)[0].all() and np.array_equal(got["idx"], ref["idx"])
    ratio = worst(np.abs(lof - ref_lof), kp.lof_bounds(ref, ref_lof, ref_lrd, 3, metric)["lof"])
    print(f"{metric}: lof of the planted row {lof[300]:.3f}, the next largest {np.delete(lof, 300).max():.3f}; err / bound {ratio:.3g}")
    assert ratio <= 1 and int(lof.argmax()) == int(ref_lof.argmax())
    if metric == "euclidean":                                           # (the cosine distance does not see how far out a row lies, only in which direction)
        assert int(lof.argmax()) == 300 and lof[300] > 2


def test_the_module_keeps_a_graph_on_the_device(ctx):
    from ganrev import knn
    from ganrev.nn_utils import DeviceTensor
    x = table(129, 3)
    raw = knn_dev(ctx, x, 10, "cosine")
    with DeviceTensor(ctx, x.shape) as t:
        ctx.upload(np.ascontiguousarray(x), t.ptr)
        for source in (x, t, (t.ptr, 129, 3)):
            g = knn.graph(ctx, source, 10)
            assert same_graph(raw, dict(idx=g.idx, dist=g.dist)) and (g.n, g.k, g.metric) == (129, 10, "cosine")
        with knn.graph(ctx, t, 10, "euclidean", rows=70, keep=True) as kept:
            first = kept.numpy()
            lof, lrd = knn.lof(ctx, kept)
            count, mean = knn.overlap(ctx, kept, first)                 # a graph on the device against its host copy
    alone = knn_dev(ctx, x[:70], 10, "euclidean")
    assert same_graph(alone, dict(idx=first.idx, dist=first.dist)) and (count == 10).all() and mean == 1.0
    ref_lof, ref_lrd = lof_dev(ctx, alone["idx"], alone["dist"])
    assert same_bits(lof, ref_lof) and same_bits(lrd, ref_lrd)


# ------------------------------------------------------------------ 6. apply_r --outliers, --mapNeighbours
BASE = ["--synthetic", "1x32x32x32", "--nbImages", "600", "--resident", "--quiet"]
NEW_FILES = ["knn_idx.npy", "knn_dist.npy", "outlier_lof.npy", "outlier_lrd.npy"]


def test_apply_r_outliers(ctx, tmp_path):
    from ganrev import apply_r, knn
    where, plain = tmp_path / "scored", tmp_path / "plain"
    summary = apply_r.main(BASE + ["--outliers", "10", "--render", "--writeTo", str(where)])
    psummary = apply_r.main(BASE + ["--writeTo", str(plain)])                                       # (without the pictures: they are not what changes)
    names = sorted(os.listdir(plain))
    assert "outliers" not in psummary and not [f for f in names if "knn" in f or "outlier" in f]
    for f in names:                                                     # every file of the run without the new options, byte for byte
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(where / f, "rb").read(), f
    timing = "embed_and_search_seconds"
    assert {q: v for q, v in summary.items() if q not in ("outliers", timing)} == {q: v for q, v in psummary.items() if q != timing}
    extra = sorted(set(os.listdir(where)) - set(names))
    assert sorted(f for f in extra if not f.endswith(".png")) == sorted(NEW_FILES) and "outliers_lof.png" in extra
    entry = json.load(open(where / "summary.json"))["outliers"]
    assert entry == summary["outliers"] and sorted(entry) == ["k", "lof_max", "lof_median", "lof_p99", "metric", "rows", "space"]
    assert (entry["k"], entry["rows"], entry["metric"], entry["space"]) == (10, 600, "cosine", "attributes")
    attributes = np.load(where / "attributes.npy")
    g = knn.graph(ctx, attributes, 10, "cosine")
    lof, lrd = knn.lof(ctx, g)
    idx, dist = np.load(where / "knn_idx.npy"), np.load(where / "knn_dist.npy")
    assert idx.shape == dist.shape == (600, 10) and idx.dtype == np.int32 and dist.dtype == np.float64
    assert same_bits(idx, g.idx) and same_bits(dist, g.dist)
    assert same_bits(np.load(where / "outlier_lof.npy"), lof) and same_bits(np.load(where / "outlier_lrd.npy"), lrd)
    assert entry["lof_max"] == float(lof.max()) and entry["lof_median"] == float(np.median(lof)) and entry["lof_median"] <= entry["lof_p99"] <= entry["lof_max"]


def test_apply_r_map_neighbours(ctx, tmp_path):
    from ganrev import apply_r
    where, plain = tmp_path / "kept", tmp_path / "plain"
    mapped = ["--map", "--mapRows", "300", "--mapIterations", "50"]
    summary = apply_r.main(BASE + mapped + ["--mapNeighbours", "10", "--writeTo", str(where)])
    psummary = apply_r.main(BASE + mapped + ["--writeTo", str(plain)])
    assert sorted(set(os.listdir(where)) - set(os.listdir(plain))) == ["map_neighbours_kept.npy"] and "neighbours" not in psummary["map"]
    for f in os.listdir(plain):
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(where / f, "rb").read(), f
    kept = np.load(where / "map_neighbours_kept.npy")
    entry = json.load(open(where / "summary.json"))["map"]["neighbours"]
    assert kept.shape == (300,) and kept.dtype == np.int32 and kept.min() >= 0 and kept.max() <= 10
    assert entry == summary["map"]["neighbours"] and (entry["k"], entry["metric"]) == (10, "cosine")
    assert entry["mean_share_kept"] == sp.chain_mean(kept / 10.0) and abs(entry["mean_share_kept"] - kept.mean() / 10) < 1e-12
    from ganrev import knn
    there, here = knn.graph(ctx, np.load(where / "attributes.npy"), 10, "cosine", rows=300), knn.graph(ctx, np.load(where / "map_y.npy"), 10, "euclidean")
    count, mean = knn.overlap(ctx, there, here)
    assert np.array_equal(kept, count) and mean == entry["mean_share_kept"]


def test_apply_r_outliers_in_the_whitened_projection(ctx, tmp_path):
    from ganrev import apply_r, knn
    where = tmp_path / "white"
    summary = apply_r.main(BASE + ["--pca", "8", "--pcaSpace", "--outliers", "10", "--outlierMetric", "euclidean", "--outlierRows", "500", "--writeTo", str(where)])
    entry = summary["outliers"]
    assert (entry["k"], entry["rows"], entry["metric"], entry["space"]) == (10, 500, "euclidean", "pca_whitened") and 0 < entry["kept_by_pca"] <= 1
    assert np.load(where / "knn_idx.npy").shape == (500, 10) and np.load(where / "outlier_lof.npy").shape == (500,)
    before = knn.graph(ctx, np.load(where / "attributes.npy"), 10, "euclidean", rows=500)
    count, mean = knn.overlap(ctx, before, knn.Graph(np.load(where / "knn_idx.npy"), np.load(where / "knn_dist.npy")))
    assert mean == entry["kept_by_pca"] and count.shape == (500,)
