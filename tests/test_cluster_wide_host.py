"""not-gpu: the restatement of gr_cluster_dev's wide route (tests/cluster_wide_paths.py) against the oracle's k-means above 32 clusters, its
grouping against numpy's stable argsort, the route rule against the sources, and ganrev.apply_r's clustering options."""
import os
import re

import numpy as np
import pytest

import cluster_wide_paths as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_route_rule_and_constants_match_the_sources():
    km = source("gan-reverser_amd", "csrc", "kmeans.hip")
    assert f"int g_cluster_wide_min_k = {cw.WIDE_MIN_K};" in km
    consts = dict(re.findall(r"\b(K[MW]_[A-Z]+) = (\d+)", km))
    rpb = re.search(r"constexpr int ROWS_PER_BLOCK = (\d+)", source("gan-reverser_amd", "csrc", "kernels.h")).group(1)      # the one constant of every family
    assert int(consts["KM_KMAX"]) == cw.NARROW_MAX_K and int(rpb) == cw.ROWS_PER_BLOCK and "KW_SEGMAX = ROWS_PER_BLOCK" in km
    assert int(consts["KW_KT"]) == cw.CENTROID_TILE and int(consts["KW_TR"]) == cw.ROWS_PER_WORKGROUP and int(consts["KW_KMAX"]) == cw.MAX_K
    assert cw.CENTROID_TILE == 8 * cw.CENTROIDS_PER_THREAD
    assert "return k >= g_cluster_wide_min_k || k > KM_KMAX || (size_t)k * d * sizeof(double) > 60 * 1024;" in km
    assert '"cluster_wide_min_k")) { gr::g_cluster_wide_min_k = value;' in source("gan-reverser_amd", "csrc", "net.hip")
    import ganrev._lib as L
    from ganrev import apply_r
    assert L.Context.CLUSTER_WIDE_MIN_K == cw.WIDE_MIN_K
    assert (apply_r.MAX_CLUSTERS, apply_r.NARROW_MAX_CLUSTERS, apply_r.MAX_PER_CLUSTER) == (cw.MAX_K, cw.NARROW_MAX_K, cw.MAX_M)
    assert "gr_cluster_dev" in L.EXPORTED_SYMBOLS
    for k, d, key, want in ((1, 3, 33, "narrow"), (32, 100, 33, "narrow"), (33, 100, 33, "wide"), (4096, 256, 33, "wide"), (20, 32, 1, "wide"),
                            (32, 256, 33, "wide"), (30, 256, 33, "narrow"), (4097, 8, 33, "unsupported"), (4, 257, 33, "unsupported")):
        assert cw.route(k, d, key) == want, (k, d, key)


def test_grouping_is_a_stable_sort_by_label():
    rng = np.random.default_rng(3)
    for n, k in ((1, 1), (37, 5), (512, 1), (513, 40), (1300, 33), (5000, 4096), (3000, 600)):
        labels = rng.integers(0, k, n).astype(np.int32)
        if k > 2:
            labels[labels == 1] = 0                                    # a cluster without a row
        order, blocks = cw.group(labels, k)
        flat = np.concatenate(order)
        assert len(flat) == n
        for b, (o, (sl, ss, nv)) in enumerate(zip(order, blocks)):
            r0 = b * cw.ROWS_PER_BLOCK
            blk = labels[r0:r0 + cw.ROWS_PER_BLOCK]
            assert np.array_equal(o - r0, np.argsort(blk, kind="stable")), (n, k, b)
            assert nv == len(blk) and np.all(np.diff(sl) > 0) and len(sl) <= cw.segment_slots(k) and np.array_equal(sl, np.unique(blk))
            ends = np.r_[ss[1:], nv]
            for lab, st, en in zip(sl, ss, ends):                      # a segment = the cluster's rows of the block, ascending
                assert np.array_equal(o[st:en], r0 + np.nonzero(blk == lab)[0])
        ints, doubles = cw.workspace_ints_and_doubles(n, 8, k)
        B = len(blocks)                                                # the index is O(n) entries whatever k: at most 1538 ints per block of 512 rows
        assert ints <= (3 * cw.ROWS_PER_BLOCK + 2) * B + n and doubles == B * min(k, cw.ROWS_PER_BLOCK) * 8
    # labels outside [0, k) belong to no cluster
    o, sl, ss = cw.group_block(np.array([3, -1, 0, 7, 3, 0], np.int32), 4)
    assert list(o) == [2, 5, 0, 4] and list(sl) == [0, 3] and list(ss) == [0, 2]


def test_first_maximum_rule():
    v = np.array([[1, 3, 3, 2], [np.nan, 5, 1, 1], [2, np.nan, 7, 7], [-np.inf, -np.inf, -np.inf, -np.inf], [0.0, -0.0, 0.0, -1]], np.float32)
    assert list(cw.first_maximum(v)) == [1, 0, 2, 0, 0]
    for row in v:                                                      # the sequential scan itself
        best, bi = row[0], 0
        for j in range(1, len(row)):
            if row[j] > best:
                best, bi = row[j], j
        assert cw.first_maximum(row[None])[0] == bi


@pytest.mark.parametrize("N,d,k,niter", cw.HOST_CASES)
def test_twin_equals_the_oracle_above_32_clusters(oracle, N, d, k, niter):
    """The oracle adds a cluster's rows in one fp64 chain, the contract in 512-row blocks: both round an fp64 sum to fp32 once, and in these four
    cases the results are the same bits (labels, total counts and centroids)."""
    x, c0 = cw.case(N, d, k)
    cent, tot, lab = cw.kmeans(x, k, niter, c0)
    rcent, rtot, rlab = oracle.kmeans(x, k, niter, c0)
    empty = k - len(np.unique(lab))                                    # in the last iteration: these kept the centroid they had
    print(f"N {N} d {d} k {k} niter {niter}: clusters without a row {empty}, max |centroid - oracle| {np.abs(cent - rcent).max():.3g}")
    assert np.array_equal(lab, rlab) and lab.dtype == rlab.dtype
    assert np.array_equal(tot, rtot)
    assert np.array_equal(cent.view(np.uint32), rcent.view(np.uint32))
    assert empty == (15 if k == 1024 else 0)


def test_apply_r_clustering_options():
    from ganrev import apply_r
    OPT = apply_r.parse(["--synthetic", "1x32x32x32"])
    assert apply_r.clusterOptions(OPT) == (20, 15, 71, False)          # apply_r.lua:159-163
    assert not {"nbClusters", "nbIterations", "nbMaxPerCluster", "closest"} & set(vars(OPT))      # a run without them is configured as it was
    OPT = apply_r.parse(["--synthetic", "1x32x32x32", "--nbClusters", "1024", "--nbIterations", "3", "--nbMaxPerCluster", "128", "--closest"])
    assert apply_r.clusterOptions(OPT) == (1024, 3, 128, True) and OPT.nbClusters == 1024
    assert apply_r.clusterOptions(apply_r.parse(["--synthetic", "1x32x32x32", "--nbClusters", "40"])) == (40, 15, 71, False)
    for bad in (["--nbMaxPerCluster", "129"], ["--nbMaxPerCluster", "0"], ["--nbClusters", "4097"], ["--nbClusters", "0"], ["--nbIterations", "-1"]):
        with pytest.raises(SystemExit):
            apply_r.parse(["--synthetic", "1x32x32x32"] + bad)
    import ganrev._lib as L
    with pytest.raises(L.GanrevError, match="4097"):
        apply_r.checkClusterCount(4097)
