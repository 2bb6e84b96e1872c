"""gpu: gr_silhouette_dev (csrc/silhouette.hip) against float64 numpy (tests/silhouette_oracle.py) within the bounds tests/silhouette_paths.py derives
from the library's operation chains - every numeric check asserts max err / bound <= 1 and prints the ratio - the rules, the bit identities, and
ganrev.apply_r --silhouette / --silhouetteSweep.  Outputs start from garbage (7)."""
import contextlib
import json
import os

import numpy as np
import pytest

import silhouette_oracle as so
import silhouette_paths as sp
from test_silhouette_host import CLUSTER_SHAPES, COLUMN_SHAPES, EDGE_SIZES, INSIDE_SIZES, ROW_SHAPES, RULE_X, case, check, sized_case

pytestmark = pytest.mark.gpu

QUANTITIES = ("values", "a", "b", "nearest", "cluster_mean", "sizes", "mean")


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


def silhouette_dev(ctx, x, labels, k, metric, optional=(True, True, True), misalign=False, n=None):
    """-> dict(values, a, b, nearest, cluster_mean, sizes, mean); a, b, nearest stay 7 where not asked for.  n: the row count passed, when it
    is not the table's (a refusal is expected)"""
    x = np.ascontiguousarray(x, np.float32)
    rows, d = x.shape
    n = rows if n is None else n
    table = np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]) if misalign else x
    outs = (np.full(rows, 7.0), np.full(rows, 7.0), np.full(rows, 7.0), np.full(rows, 7, np.int32), np.full(k, 7.0), np.full(k, 7, np.int32), np.full(1, 7.0))
    with on_device(ctx, table, np.asarray(labels, np.int32), *outs) as (dx, dl, ds, da, db, dn, dcm, dsz, dm):
        ctx.silhouette_dev(dx + 4 if misalign else dx, n, d, dl, k, metric, ds, dcm, dsz, dm, da if optional[0] else None, db if optional[1] else None,
                           dn if optional[2] else None)
        return dict(values=ctx.download(ds, (rows,), np.float64), a=ctx.download(da, (rows,), np.float64), b=ctx.download(db, (rows,), np.float64),
                    nearest=ctx.download(dn, (rows,), np.int32), cluster_mean=ctx.download(dcm, (k,), np.float64), sizes=ctx.download(dsz, (k,), np.int32),
                    mean=float(ctx.download(dm, (1,), np.float64)[0]))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b, quantities=QUANTITIES):
    return all(np.array_equal(bits(np.asarray(a[q])), bits(np.asarray(b[q]).astype(np.asarray(a[q]).dtype))) for q in quantities)


# ------------------------------------------------------------------ 1. against the oracle, within the bounds
@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("n,d,k", ROW_SHAPES + COLUMN_SHAPES + CLUSTER_SHAPES)
def test_against_the_oracle(ctx, n, d, k, metric):
    x, labels = case(n, d, k)
    got = silhouette_dev(ctx, x, labels, k, metric)
    check(got, (n, d, k), metric)


@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("sizes", [EDGE_SIZES, INSIDE_SIZES], ids=["clusters_end_at_tile_edges", "three_clusters_end_inside_one_tile"])
def test_clusters_that_end_at_and_inside_the_tiles(ctx, sizes, metric):
    x, labels = sized_case(sizes)
    check(silhouette_dev(ctx, x, labels, len(sizes), metric), ("sizes", sizes), metric)


@pytest.mark.parametrize("metric", so.METRICS)
@pytest.mark.parametrize("key", [(65, 3, 3), (130, 33, 4), (513, 3, 3), (200, 5, 4096), ("sizes", INSIDE_SIZES)], ids=str)
def test_the_restated_chain_gives_the_devices_bits(ctx, key, metric):
    """the order of every chain - columns, members, clusters, blocks - is the one the header states: tests/silhouette_paths.py, which performs
    those operations in that order in numpy, agrees bit for bit"""
    x, labels = sized_case(key[1]) if key[0] == "sizes" else case(*key)
    k = len(key[1]) if key[0] == "sizes" else key[2]
    assert same_bits(silhouette_dev(ctx, x, labels, k, metric), sp.chain(x, labels, k, metric))


# ------------------------------------------------------------------ 2. the rules
def agrees_with_the_rules(ctx, x, labels, k, metric):
    got, ref = silhouette_dev(ctx, x, labels, k, metric), sp.chain(x, labels, k, metric)
    assert same_bits(got, ref), (got, ref)
    return got


@pytest.mark.parametrize("metric", so.METRICS)
def test_singletons_and_an_empty_cluster(ctx, metric):
    got = agrees_with_the_rules(ctx, RULE_X, [0, 0, 0, 1, 1, 2], 4, metric)
    assert got["values"][5] == 0 and got["a"][5] == 0 and got["nearest"][5] >= 0 and got["b"][5] > 0
    assert got["sizes"].tolist() == [3, 2, 1, 0] and got["cluster_mean"][2] == 0 and got["cluster_mean"][3] == 0


@pytest.mark.parametrize("metric", so.METRICS)
def test_labels_of_minus_one_and_k_are_no_cluster(ctx, metric):
    got = agrees_with_the_rules(ctx, RULE_X, [0, 0, -1, 1, 1, 4], 4, metric)
    assert got["sizes"].tolist() == [2, 2, 0, 0] and got["nearest"][[2, 5]].tolist() == [-1, -1]
    assert not got["values"][[2, 5]].any() and not got["a"][[2, 5]].any() and not got["b"][[2, 5]].any()
    inside = silhouette_dev(ctx, RULE_X[[0, 1, 3, 4]], [0, 0, 1, 1], 4, metric)      # such rows are nobody's member: the others score as without them
    assert np.array_equal(bits(got["values"][[0, 1, 3, 4]]), bits(inside["values"]))


@pytest.mark.parametrize("metric", so.METRICS)
def test_one_cluster_alone_scores_zero(ctx, metric):
    got = agrees_with_the_rules(ctx, RULE_X, [0] * 6, 1, metric)
    assert not got["values"].any() and (got["nearest"] == -1).all() and not got["b"].any() and (got["a"] > 0).all() and got["mean"] == 0


def test_duplicate_rows_have_a_zero(ctx):
    x = np.repeat(np.array([[0.5, -1.25, 3.0], [2.0, 2.0, -1.0]], np.float32), [3, 4], axis=0)
    got = agrees_with_the_rules(ctx, x, [0, 0, 0, 1, 1, 1, 1], 2, "euclidean")
    assert not got["a"].any() and (got["b"] > 0).all() and (got["values"] == 1).all() and got["mean"] == 1


def test_a_zero_row_under_the_cosine_distance(ctx):
    x = np.array([[0, 0], [1, 0], [2, 0], [0, 3]], np.float32)
    got = agrees_with_the_rules(ctx, x, [0, 0, 1, 1], 2, "cosine")
    assert got["a"][0] == 1 and got["b"][0] == 1 and got["values"][0] == 0 and got["a"][1] == 1 and got["b"][1] == 0.5


def test_exact_ties_on_integer_data(ctx):
    """points t (3, 4): every distance is a multiple of 5 and every sum exact, so a, b, s are float64 numpy's bits whatever the order; a tie in b
    goes to the lower cluster"""
    t = np.concatenate([[-10, -9, 0, 0, 9, 10], np.arange(100, 170), np.arange(-170, -100)]).astype(np.float32)
    x = t[:, None] * np.array([[3, 4]], np.float32)
    labels = np.concatenate([[2, 2, 1, 1, 0, 0], np.full(70, 3), np.full(70, 4)])
    got, ref = silhouette_dev(ctx, x, labels, 5, "euclidean"), so.silhouette(x, labels, 5, "euclidean")
    assert same_bits(got, ref, ("a", "b", "values", "nearest", "sizes"))
    assert got["a"][2] == 0 and got["b"][2] == 47.5 and got["nearest"][2] == 0 and got["nearest"][3] == 0      # clusters 0 and 2 tie for rows 2 and 3


# ------------------------------------------------------------------ 3. bit identities
def test_two_runs_agree(ctx):
    x, labels = case(513, 3, 3)
    for metric in so.METRICS:
        assert same_bits(silhouette_dev(ctx, x, labels, 3, metric), silhouette_dev(ctx, x, labels, 3, metric))


def test_table_pointer_offset_by_four_bytes(ctx):
    x, labels = case(130, 100, 4)
    for metric in so.METRICS:
        assert same_bits(silhouette_dev(ctx, x, labels, 4, metric), silhouette_dev(ctx, x, labels, 4, metric, misalign=True))


def test_optional_outputs_left_out_leave_the_others_unchanged(ctx):
    x, labels = case(129, 3, 3)
    whole = silhouette_dev(ctx, x, labels, 3, "cosine")
    for optional in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        part = silhouette_dev(ctx, x, labels, 3, "cosine", optional=optional)
        assert same_bits(whole, part, ("values", "cluster_mean", "sizes", "mean"))
        for q, asked in zip(("a", "b", "nearest"), optional):
            assert np.array_equal(bits(part[q]), bits(whole[q])) if asked else (part[q] == 7).all()


def test_one_row_too_many_is_refused_by_name_and_the_next_call_works(ctx):
    import ganrev._lib as L
    x, labels = case(63, 3, 3)
    before = silhouette_dev(ctx, x, labels, 3, "euclidean")
    with pytest.raises(L.GanrevError, match="262145"):
        silhouette_dev(ctx, x, labels, 3, "euclidean", n=262145)        # refused before anything is read
    for bad, word in ((dict(n=1), "n 1"), (dict(k=4097), "4097")):
        with pytest.raises(L.GanrevError, match=word):
            silhouette_dev(ctx, x, labels, bad.get("k", 3), "euclidean", n=bad.get("n"))
    with pytest.raises(L.GanrevError, match="metric 2"):
        silhouette_dev(ctx, x, labels, 3, 2)
    assert same_bits(before, silhouette_dev(ctx, x, labels, 3, "euclidean"))


def test_score_takes_a_host_array_a_device_tensor_or_a_pointer(ctx):
    from ganrev import silhouette
    from ganrev.nn_utils import DeviceTensor
    x, labels = case(129, 3, 3)
    raw = silhouette_dev(ctx, x, labels, 3, "cosine")
    with DeviceTensor(ctx, x.shape) as t:
        ctx.upload(np.ascontiguousarray(x), t.ptr)
        for table in (x, t, (t.ptr, 129, 3)):
            sc = silhouette.score(ctx, table, labels, 3)
            assert same_bits(raw, dict(values=sc.values, a=sc.a, b=sc.b, nearest=sc.nearest, cluster_mean=sc.cluster_mean, sizes=sc.sizes, mean=sc.mean))
        first = silhouette.score(ctx, t, labels[:70], 3, "euclidean", rows=70)      # a prefix: later rows are nobody's member
    assert same_bits(silhouette_dev(ctx, x[:70], labels[:70], 3, "euclidean"), dict(values=first.values, mean=first.mean), ("values", "mean"))


# ------------------------------------------------------------------ 4. apply_r --silhouette, --silhouetteSweep
BASE = ["--synthetic", "1x32x32x32", "--nbImages", "600", "--resident", "--quiet"]
NEW_FILES = ["silhouette_%s_%s.npy" % (name, metric) for name in ("clusters", "mixture") for metric in so.METRICS]


def test_apply_r_silhouette(ctx, tmp_path):
    from ganrev import apply_r, silhouette
    where, plain = tmp_path / "scored", tmp_path / "plain"
    summary = apply_r.main(BASE + ["--mixture", "2", "--silhouette", "--silhouetteSweep", "4,8", "--writeTo", str(where)])
    psummary = apply_r.main(BASE + ["--mixture", "2", "--writeTo", str(plain)])
    names = sorted(os.listdir(plain))
    assert "silhouette" not in psummary and not [f for f in names if "silhouette" in f]
    for f in names:                                                     # every file of the run without the new options, byte for byte
        if f != "summary.json":
            assert open(plain / f, "rb").read() == open(where / f, "rb").read(), f
    timing = "embed_and_search_seconds"
    assert {q: v for q, v in summary.items() if q not in ("silhouette", timing)} == {q: v for q, v in psummary.items() if q != timing}
    assert sorted(set(os.listdir(where)) - set(names)) == sorted(NEW_FILES + ["silhouette_clusters_labels.npy", "silhouette_sweep.json"])
    entry = json.load(open(where / "summary.json"))["silhouette"]
    assert entry == summary["silhouette"] and entry["rows"] == 600 and entry["space"] == "attributes"
    attributes, centroids = np.load(where / "attributes.npy"), np.load(where / "cluster_centroids.npy")
    cluster_labels = np.load(where / "silhouette_clusters_labels.npy")
    assert np.array_equal(cluster_labels, ctx.cosine_assign(attributes, centroids, take_min=True)[0])       # the clustering's own assignment (apply_r.lua:205-217)
    for name, labels in (("clusters", cluster_labels), ("mixture", np.load(where / "mixture_labels.npy"))):
        for metric in so.METRICS:
            sc = silhouette.score(ctx, attributes, labels, 20, metric)
            assert np.array_equal(bits(np.load(where / ("silhouette_%s_%s.npy" % (name, metric)))), bits(sc.values))
            assert entry[name][metric] == sc.summary() and len(entry[name][metric]["sizes"]) == 20 and -1 <= sc.mean <= 1
    sweep = json.load(open(where / "silhouette_sweep.json"))
    assert [e["K"] for e in sweep["sweep"]] == [4, 8] and sweep["rows"] == 600
    for e in sweep["sweep"]:
        assert -1 <= e["mean_euclidean"] <= 1 and -1 <= e["mean_cosine"] <= 1 and 0 <= e["empty_clusters"] < e["K"]
