"""gpu: gr_cluster_dev (apply_r.lua:198-227 in one enqueue, up to 4096 clusters).  Its wide kernels against the three k <= 32 calls bit for bit
(the tuning key "cluster_wide_min_k" forced to 1), above 32 clusters against the oracle and the numpy member selection (tests/cluster_oracle.py),
the first maximum across the wide kernel's tiles, ties and NaN through the data, the limits, determinism, and ganrev.apply_r --nbClusters.
A run of apply_r without the new options makes the calls it made before: tests/test_gpu_apply_r_resident.py, test_gpu_embed.py and
test_gpu_imagegrid.py hold those files, so nothing here repeats them."""
import contextlib
import functools
import json

import numpy as np
import pytest

import cluster_oracle as clo
import cluster_wide_paths as cw

pytestmark = pytest.mark.gpu
KEY = "cluster_wide_min_k"
NAMES = ("centroids", "total counts", "labels", "sims", "rows", "row sims", "kept", "sizes")


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


@contextlib.contextmanager
def wide_from(ctx, k):
    ctx.set_tuning(KEY, k)
    try:
        yield
    finally:
        ctx.set_tuning(KEY, cw.WIDE_MIN_K)


def outputs(n, k, m):
    return (np.full(k, 7, np.float32), np.full(n, 7, np.int32), np.full(n, 7, np.float32), np.full((k, m), 7, np.int64), np.full((k, m), 7, np.float32),
            np.full(k, 7, np.int32), np.full(k, 7, np.int32))


def download(ctx, ptrs, n, d, k, m):
    dc, dt, dl, ds, dr, drs, dk, dz = ptrs
    return (ctx.download(dc, (k, d)), ctx.download(dt, (k,)), ctx.download(dl, (n,), np.int32), ctx.download(ds, (n,)),
            ctx.download(dr, (k, m), np.int64), ctx.download(drs, (k, m)), ctx.download(dk, (k,), np.int32), ctx.download(dz, (k,), np.int32))


def cluster_dev(ctx, x, k, niter, c0, take_min, m, dx=None):
    n, d = x.shape
    with on_device(ctx, c0, *outputs(n, k, m)) as ptrs, (contextlib.nullcontext([dx]) if dx else on_device(ctx, x)) as (px,):
        dc, dt, dl, ds, dr, drs, dk, dz = ptrs
        ctx.cluster_dev(px, n, d, k, niter, dc, take_min, m, dt, dl, ds, dr, drs, dk, dz)
        return download(ctx, ptrs, n, d, k, m)


def chained(ctx, x, k, niter, c0, take_min, m, dx):
    """the three k <= 32 calls, as apply_r made them before gr_cluster_dev"""
    n, d = x.shape
    with on_device(ctx, c0, *outputs(n, k, m)) as ptrs:
        dc, dt, dl, ds, dr, drs, dk, dz = ptrs
        ctx.kmeans_dev(dx, n, d, k, niter, dc, dt, dl)
        ctx.cosine_assign_dev(dx, n, d, dc, k, take_min, dl, ds)
        ctx.cluster_members_dev(dl, ds, n, k, m, dr, drs, dk, dz)
        return download(ctx, ptrs, n, d, k, m)


def same_bytes(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


def data(N, d, k, seed=71):
    from ganrev import synth
    x = synth.normal((N, d), seed)
    x[: N // 3] += 1.5
    c0 = synth.normal((k, d), seed + 1)
    c0 /= np.linalg.norm(c0, axis=1, keepdims=True)
    return x, c0.astype(np.float32)


# ------------------------------------------------------------------ 1. wide = narrow, bit for bit
@pytest.mark.parametrize("d", [3, 32, 33, 100])
@pytest.mark.parametrize("N", [37, 512, 513, 1300])
def test_wide_route_equals_the_three_calls(ctx, N, d):
    """N: one ragged block, exactly one, a one-row second block, three blocks (and 1, 4, 5, 11 workgroups of the wide assignment); d: around the
    32-column staging boundary; k: one centroid, two and three half-waves' share of a centroid tile"""
    m = 71
    for k in (1, 20, 32):
        x, c0 = data(N, d, k)
        assert cw.route(k, d) == "narrow" and cw.route(k, d, 1) == "wide"
        with on_device(ctx, x) as (dx,):
            for niter in (0, 3):
                for take_min in (0, 1):
                    want = chained(ctx, x, k, niter, c0, take_min, m, dx)
                    with wide_from(ctx, 1):
                        same_bytes(cluster_dev(ctx, x, k, niter, c0, take_min, m, dx), want, ("wide", N, d, k, niter, take_min))
                    same_bytes(cluster_dev(ctx, x, k, niter, c0, take_min, m, dx), want, ("default key", N, d, k, niter, take_min))


def test_wide_route_widest_rows_and_a_nan_row(ctx):
    """d = 256 (the wide assignment holds 128 x 257 floats in LDS; the narrow accumulate kernel fits 30 clusters), and a row with a NaN element:
    label 0 in the k-means, so centroid 0 turns NaN and, as in the three calls, draws every row in the assignment that follows"""
    x, c0 = data(700, 256, 30)
    with on_device(ctx, x) as (dx,):
        want = chained(ctx, x, 30, 2, c0, 1, 71, dx)
        with wide_from(ctx, 1):
            same_bytes(cluster_dev(ctx, x, 30, 2, c0, 1, 71, dx), want, "d = 256")
    x, c0 = data(1300, 33, 20)
    x[777, 5] = np.nan
    with on_device(ctx, x) as (dx,):
        want = chained(ctx, x, 20, 1, c0, 1, 71, dx)
        with wide_from(ctx, 1):
            got = cluster_dev(ctx, x, 20, 1, c0, 1, 71, dx)
    assert np.isnan(want[0][0]).any() and (want[2] == 0).all() and np.isnan(want[3]).all()
    for g, w, name in zip(got, want, NAMES):                            # a NaN is a NaN whatever its payload; everything else bit for bit
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.dtype == np.float32:
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g.view(np.uint32)[~np.isnan(g)], w.view(np.uint32)[~np.isnan(w)]), name
        else:
            assert np.array_equal(g, w), name


# ------------------------------------------------------------------ 2. above 32 clusters against the oracle
@functools.lru_cache(maxsize=None)
def oracle_kmeans(N, d, k, niter):
    from oracle import oracle as o
    o.build()
    x, c0 = cw.case(N, d, k)
    return (x, c0) + tuple(o.kmeans(x, k, niter, c0))


@pytest.mark.parametrize("N,d,k,niter", cw.HOST_CASES + cw.GPU_ONLY_CASES)
def test_above_32_clusters_against_the_oracle(ctx, oracle, N, d, k, niter):
    """(700, 256, 64): the widest rows; (5000, 8, 4096): most clusters empty, 32 centroid tiles; (70001, 8, 257): 137 row blocks, so a cluster's
    workgroup looks its segments up in more than one pass of 256 blocks.  Counts exactly (the k-means labels follow from them), centroids to the
    1e-6 of test_kmeans_and_cluster_assignment, the cosine assignment on the device's centroids exactly, the member lists exactly."""
    x, c0, rcent, rtot, _ = oracle_kmeans(N, d, k, niter)
    assert cw.route(k, d) == "wide"
    m = 71
    with on_device(ctx, x) as (dx,):
        for take_min in (1, 0):
            cent, tot, lab, sim, rows, rsim, kept, sizes = cluster_dev(ctx, x, k, niter, c0, take_min, m, dx)
            worst = float(np.abs(cent - rcent).max())
            print(f"N {N} d {d} k {k} niter {niter}: max |centroid - oracle| {worst:.3g}, bit-equal {np.array_equal(cent.view(np.uint32), rcent.view(np.uint32))}")
            assert np.array_equal(tot, rtot) and tot.dtype == rtot.dtype
            assert worst <= 1e-6
            rla, rsi = oracle.cosine_assign(x, cent, bool(take_min))
            assert np.array_equal(lab, rla) and np.array_equal(sim.view(np.uint32), rsi.view(np.uint32))
            for g, w, name in zip((rows, rsim, kept, sizes), clo.cluster_members(lab, sim, k, m), NAMES[4:]):
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
            assert sizes.sum() == N


# ------------------------------------------------------------------ 3. the first maximum across tiles
@pytest.mark.parametrize("k,pairs", [(64, ((3, 3 + cw.CENTROIDS_PER_THREAD), (5, 5 + 3 * cw.CENTROIDS_PER_THREAD))),
                                      (2 * cw.CENTROID_TILE + 2, ((3, 3 + cw.CENTROID_TILE), (1, 1 + 2 * cw.CENTROID_TILE)))])
def test_first_maximum_across_tiles_and_unchosen_centroid(ctx, k, pairs):
    """Two identical centroids: the first maximum wins, the later one never gets a row and keeps its value; a centroid far from every row keeps its
    value too (mirrors test_kmeans_dev_first_maximum_and_unchosen_centroid).  The wide kernel stages cw.CENTROID_TILE centroids per tile and gives
    each half-wave cw.CENTROIDS_PER_THREAD of them, so at k = 64 the copies sit in different half-waves' shares of the one tile - where the kernel
    merges running maxima - and at two tiles + 2 in different staged tiles."""
    x, c0 = data(1300, 32, k)
    far = 11
    for a, b in pairs:
        c0[b] = c0[a]
    c0[far] = -40.0 * np.abs(c0[far]) - 40.0
    cent, tot, lab, sim, rows, rsim, kept, sizes = cluster_dev(ctx, x, k, 1, c0, 0, 71)
    scores = cw.scores(x, c0, cw.c2_of(c0))
    want = cw.first_maximum(scores)
    assert np.array_equal(tot, np.bincount(want, minlength=k).astype(np.float32))
    for a, b in pairs:
        assert tot[b] == 0 and np.array_equal(cent[b], c0[b]) and np.array_equal(scores[:, a], scores[:, b])
    assert tot[far] == 0 and np.array_equal(cent[far], c0[far])
    assert any(tot[a] > 0 for a, _ in pairs)
    tw, _, _ = cw.kmeans(x, k, 1, c0)
    assert np.array_equal(cent.view(np.uint32), tw.view(np.uint32))


# ------------------------------------------------------------------ 4. ties and NaN through the data
def test_ties_and_nan_through_the_data(ctx, oracle):
    N, d, k, m = 900, 16, 40, 71
    x, c0 = data(N, d, k, seed=5)
    same = np.arange(10, 810, 10)                                       # eighty identical rows, next to centroid 7
    x[same] = 6.0 * c0[7]
    cent, tot, lab, sim, rows, rsim, kept, sizes = cluster_dev(ctx, x, k, 2, c0, 0, m)
    j = lab[same[0]]
    assert (lab[same] == j).all() and len(set(sim[same].view(np.uint32).tolist())) == 1 and sizes[j] >= 80 and kept[j] == m
    assert sim[same[0]] >= sim[lab == j].max()
    assert np.array_equal(rows[j], same[:m])                           # the first 71 of the eighty by row index
    for g, w in zip((rows, rsim, kept, sizes), clo.cluster_members(lab, sim, k, m)):
        assert g.tobytes() == w.tobytes()
    # a NaN element: label 0 and a NaN similarity; it ranks last in cluster 0 (no iteration: the centroids stay finite)
    x[333, 4] = np.nan
    cent, tot, lab, sim, rows, rsim, kept, sizes = cluster_dev(ctx, x, k, 0, c0, 0, 128)
    assert lab[333] == 0 and np.isnan(sim[333]) and np.isnan(sim).sum() == 1 and np.array_equal(cent, c0) and not tot.any()
    want = clo.cluster_members(lab, sim, k, 128)
    assert np.array_equal(rows, want[0]) and np.array_equal(kept, want[2]) and np.array_equal(sizes, want[3])
    assert sizes[0] <= 128 and rows[0, kept[0] - 1] == 333 and np.isnan(rsim[0, kept[0] - 1]) and not np.isnan(rsim[0, :kept[0] - 1]).any()
    rla, rsi = oracle.cosine_assign(x, c0, False)
    assert np.array_equal(lab, rla) and np.array_equal(np.isnan(sim), np.isnan(rsi))


# ------------------------------------------------------------------ 5. limits
def test_limits(ctx):
    import ganrev._lib as L
    x, c0 = data(64, 8, 4)
    for (n, d, k, m), code, word in (((64, 8, 4097, 8), "GR_ERR_UNSUPPORTED", "4097"), ((64, 257, 4, 8), "GR_ERR_UNSUPPORTED", "257"),
                                     ((64, 8, 4, 129), "GR_ERR_UNSUPPORTED", "129"), ((0, 8, 4, 8), "GR_ERR_INVALID", "n 0")):
        big = np.zeros((64, max(d, 8)), np.float32)
        with on_device(ctx, big, np.zeros((k, d), np.float32), *outputs(64, k, m)) as (dx, dc, dt, dl, ds, dr, drs, dk, dz):
            with pytest.raises(L.GanrevError, match=code) as e:
                ctx.cluster_dev(dx, n, d, k, 1, dc, 1, m, dt, dl, ds, dr, drs, dk, dz)
            assert word in str(e.value), str(e.value)
    with on_device(ctx, x) as (dx,):                                   # the context stays usable
        same_bytes(cluster_dev(ctx, x, 4, 2, c0, 1, 8, dx), chained(ctx, x, 4, 2, c0, 1, 8, dx), "after the refusals")
    x, c0 = cw.case(1300, 33, 33)
    got = cluster_dev(ctx, x, 33, 3, c0, 1, 71)
    assert np.array_equal(got[1], oracle_kmeans(1300, 33, 33, 3)[3])


# ------------------------------------------------------------------ 6. determinism
def test_two_runs_agree_bit_for_bit(ctx):
    x, c0 = cw.case(5000, 33, 257)
    with on_device(ctx, x) as (dx,):
        same_bytes(cluster_dev(ctx, x, 257, 3, c0, 1, 71, dx), cluster_dev(ctx, x, 257, 3, c0, 1, 71, dx), "second run")


# ------------------------------------------------------------------ 7. the script
def test_apply_r_nbClusters_40(ctx, oracle, tmp_path):
    from ganrev import apply_r, synth
    from ganrev.nn_utils import DeviceTensor
    k, m, seed = 40, 71, 1
    summary = apply_r.main(["--synthetic", "1x32x32x32", "--nbImages", "600", "--nbClusters", str(k), "--resident", "--quiet", "--writeTo", str(tmp_path)])
    assert (summary["nbClusters"], summary["nbIterations"], summary["nbMaxPerCluster"], summary["closest"]) == (k, 15, m, False)
    assert json.load(open(tmp_path / "summary.json"))["nbClusters"] == k
    attrs = np.load(tmp_path / "attributes.npy")
    cent_file = np.load(tmp_path / "cluster_centroids.npy")
    assert cent_file.shape == (k, 32) and np.load(tmp_path / "cluster_average_faces.npy").shape == (k, 1, 32, 32)
    images = synth.uniform((600, 1, 8, 8), 82, 0, 1)
    di, da = DeviceTensor(ctx, images.shape), DeviceTensor(ctx, attrs.shape)
    ctx.upload(images, di.ptr); ctx.upload(attrs, da.ptr)
    try:
        res = []
        for table in (attrs, da):                                      # the host-table route uploads the table; the device route takes it where it is
            cent, counts, clusters, faces = apply_r.createClusterImagesDev(k, 15, m, di, table, seed=seed)
            res.append((cent, counts, clusters, faces.numpy()))
            faces.free()
    finally:
        di.free(); da.free()
    (c0, n0, l0, f0), (c1, n1, l1, f1) = res
    assert np.array_equal(c0.view(np.uint32), c1.view(np.uint32)) and np.array_equal(n0, n1) and l0 == l1 and np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert np.array_equal(c0.view(np.uint32), cent_file.view(np.uint32))                    # what the script wrote
    assert summary["cluster_total_counts"] == [float(v) for v in n0] and summary["cluster_sizes"] == [len(c) for c in l0]
    hc, hn, hl, hf = apply_r.createClusterImages(k, 15, m, images, attrs, seed=seed)       # host images: the same lists, faces averaged in float64
    assert np.array_equal(hc, c0) and np.array_equal(hn, n0) and hl == l0
    # the oracle composition of test_create_cluster_images_mirror
    init = apply_r.initialCentroids(k, 32, seed)
    rcent, rtot, _ = oracle.kmeans(attrs, k, 15, init)
    assert float(np.abs(c0 - rcent).max()) <= 1e-6 and np.array_equal(n0, rtot)
    rla, rsi = oracle.cosine_assign(attrs, c0, True)
    for j, members in enumerate(l0):
        rws = np.nonzero(rla == j)[0]
        ref = rws[np.argsort(-rsi[rws], kind="stable")][:m]
        assert [r for r, _ in members] == list(ref)
        if len(ref):
            assert float(np.abs(f0[j] - images[ref].mean(0)).max()) <= 1e-6 and float(np.abs(hf[j] - images[ref].mean(0)).max()) <= 1e-6
    assert sum(len(c) for c in l0) > 0
