"""gpu: the clustering on device-resident tables (gr_kmeans_dev, gr_cosine_assign_dev, gr_cluster_members_dev, gr_cluster_faces_dev and
apply_r.createClusterImagesDev with a device attribute table) against the host-table calls the oracle pins, the numpy restatement of the
member selection (tests/cluster_oracle.py) and gr_rows_mean_dev - everything bit for bit."""
import contextlib

import numpy as np
import pytest

import cluster_oracle as clo

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            ctx.free(p)


def data(N, d, k, seed=71):
    from ganrev import synth
    x = synth.normal((N, d), seed)
    x[: N // 3] += 1.5                                # some structure so that clusters differ in size
    c0 = synth.normal((k, d), seed + 1)
    c0 /= np.linalg.norm(c0, axis=1, keepdims=True)
    return x, c0.astype(np.float32)


def kmeans_dev(ctx, x, k, niter, c0):
    n, d = x.shape
    with on_device(ctx, x, c0, np.zeros(k, np.float32), np.zeros(n, np.int32)) as (dx, dc, dt, dl):
        ctx.kmeans_dev(dx, n, d, k, niter, dc, dt, dl)
        return ctx.download(dc, (k, d)), ctx.download(dt, (k,)), ctx.download(dl, (n,), np.int32)


def same_kmeans(ctx, x, k, niter, c0, what):
    got, want = kmeans_dev(ctx, x, k, niter, c0), ctx.kmeans(x, k, niter, c0)
    for g, w, name in zip(got, want, ("centroids", "total counts", "labels")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)
    return got


@pytest.mark.parametrize("d", [3, 32, 33, 100])
@pytest.mark.parametrize("N", [37, 512, 513, 1300])
def test_kmeans_dev_is_kmeans_host(ctx, N, d):
    """N: one ragged block, exactly one block, a one-row second block, three blocks of 512 rows; d: around the 32-column staging boundary"""
    for k in (1, 20, 32):
        x, c0 = data(N, d, k)
        for niter in (0, 3):
            same_kmeans(ctx, x, k, niter, c0, (N, d, k, niter))


def test_kmeans_dev_widest_rows(ctx):
    """d = 256, the widest table the call takes: every thread of the member sums owns a column"""
    x, c0 = data(700, 256, 20)
    same_kmeans(ctx, x, 20, 2, c0, "d = 256")


def test_kmeans_dev_first_maximum_and_unchosen_centroid(ctx):
    x, c0 = data(1300, 32, 20)
    c0[7] = c0[3]                                     # two identical centroids: the first maximum wins, 7 never gets a row
    c0[11] = -40.0 * np.abs(c0[11]) - 40.0            # far away from every row: nobody chooses it
    same_kmeans(ctx, x, 20, 3, c0, "ties, three iterations")
    cent, tot, lab = same_kmeans(ctx, x, 20, 1, c0, "ties")           # one iteration: the labels are those of the initial centroids
    assert not (lab == 7).any() and not (lab == 11).any() and tot[7] == 0 and tot[11] == 0
    assert np.array_equal(cent[11], c0[11]) and np.array_equal(cent[7], c0[7])      # kept their values
    assert (lab == 3).any()


def test_kmeans_dev_limits(ctx):
    import ganrev._lib as L
    for k, d in ((33, 8), (4, 257)):
        x, c0 = data(64, d, k)
        with pytest.raises(L.GanrevError, match="GR_ERR_UNSUPPORTED"):
            kmeans_dev(ctx, x, k, 1, c0)
    x, c0 = data(64, 8, 4)
    same_kmeans(ctx, x, 4, 2, c0, "after the refusals")          # the context stays usable


@pytest.mark.parametrize("d", [3, 32, 33, 100])
@pytest.mark.parametrize("N", [37, 512, 513, 1300])
def test_cosine_assign_dev_is_cosine_assign_host(ctx, N, d):
    for k in (1, 20, 32):
        x, c0 = data(N, d, k, seed=91)
        with on_device(ctx, x, c0, np.zeros(N, np.int32), np.zeros(N, np.float32)) as (dx, dc, dl, ds):
            for take_min in (False, True):
                ctx.cosine_assign_dev(dx, N, d, dc, k, take_min, dl, ds)
                la, si = ctx.download(dl, (N,), np.int32), ctx.download(ds, (N,))
                rla, rsi = ctx.cosine_assign(x, c0, take_min)
                assert np.array_equal(la, rla) and np.array_equal(si.view(np.uint32), rsi.view(np.uint32)), (N, d, k, take_min)


def members_dev(ctx, labels, sims, k, m):
    n = len(labels)
    with on_device(ctx, labels, sims, np.full((k, m), 7, np.int64), np.full((k, m), 7, np.float32), np.full(k, 7, np.int32),
                   np.full(k, 7, np.int32)) as (dl, ds, dr, drs, dk, dz):
        ctx.cluster_members_dev(dl, ds, n, k, m, dr, drs, dk, dz)
        return (ctx.download(dr, (k, m), np.int64), ctx.download(drs, (k, m)), ctx.download(dk, (k,), np.int32), ctx.download(dz, (k,), np.int32))


def same_members(got, want, what):
    for g, w, name in zip(got, want, ("rows", "sims", "kept", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bits = (lambda a: a.view(np.uint32)) if g.dtype == np.float32 else (lambda a: a)
        if name == "sims":                            # a NaN is a NaN whatever its payload; every other value bit for bit (-0 is not +0)
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(bits(g)[~np.isnan(g)], bits(w)[~np.isnan(w)]), (what, name)
        else:
            assert np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("m", [1, 71, 128])
@pytest.mark.parametrize("k", [1, 20, 32])
@pytest.mark.parametrize("N", [37, 1300, 5000])
def test_cluster_members_dev(ctx, N, k, m):
    nan = (N, k, m) == (1300, 20, 71)
    labels, sims = clo.member_case(N, k, m, seed=N + k + m, nan=nan)
    if k > 1:
        assert not (labels == k - 1).any()
    assert (labels == 0).sum() > m or N <= m + 9
    got = members_dev(ctx, labels, sims, k, m)
    same_members(got, clo.cluster_members(labels, sims, k, m), (N, k, m))
    again = members_dev(ctx, labels, sims, k, m)
    for g, a in zip(got, again):
        assert g.tobytes() == a.tobytes()             # two runs agree bit for bit


def test_cluster_members_dev_many_row_ranges(ctx):
    """200 000 rows: the rows are shared among several workgroups per cluster and their lists merged; distinct similarities with a block
    of exact ties across the cut-off and NaNs"""
    N, k, m = 200000, 20, 71
    rng = np.random.default_rng(5)
    labels = rng.integers(0, k - 1, N).astype(np.int32)
    sims = rng.standard_normal(N).astype(np.float32)
    top = np.nonzero(labels == 2)[0]
    sims[top[::7][:300]] = 9.0                        # 300 equal leaders in cluster 2: the first 71 rows of them are kept
    sims[rng.permutation(N)[:50]] = np.nan
    got = members_dev(ctx, labels, sims, k, m)
    same_members(got, clo.cluster_members(labels, sims, k, m), "200000 rows")
    assert (got[1][2] == 9.0).all()


@pytest.mark.parametrize("N,m", [(600000, 128), (140000, 1), (140000, 128)])
def test_cluster_members_dev_row_ranges_and_m(ctx, N, m):
    """eight row ranges per cluster (600 000 rows) and two (140 000), with the longest and the shortest list; tie values from member_case"""
    k = 20
    labels, sims = clo.member_case(N, k, m, seed=N + m, nan=True)
    same_members(members_dev(ctx, labels, sims, k, m), clo.cluster_members(labels, sims, k, m), (N, k, m))


def test_cluster_members_dev_limits(ctx):
    import ganrev._lib as L
    labels, sims = clo.member_case(100, 4, 8, seed=1)
    for k, m in ((4, 129), (33, 8)):
        with pytest.raises(L.GanrevError, match="GR_ERR_UNSUPPORTED"):
            members_dev(ctx, labels, sims, k, m)
    same_members(members_dev(ctx, labels, sims, 4, 8), clo.cluster_members(labels, sims, 4, 8), "after the refusals")


@pytest.mark.parametrize("chw", [1024, 12288])
def test_cluster_faces_dev_is_rows_mean(ctx, chw):
    from ganrev import synth
    n_rows, k, m = 150, 4, 71
    table = synth.normal((n_rows, chw), 31)
    rng = np.random.default_rng(chw)
    kept = np.array([0, 1, 71, 40], np.int32)         # an empty cluster, a single row, a full list, a part of one
    rows = np.full((k, m), -1, np.int64)
    for j in range(k):
        rows[j, :kept[j]] = rng.integers(0, n_rows, kept[j])
    with on_device(ctx, table, rows, kept, np.full((k, chw), 7, np.float32), np.full((chw,), 7, np.float32)) as (dt, dr, dk, do, d1):
        ctx.cluster_faces_dev(dt, n_rows, chw, dr, dk, k, m, do)
        faces = ctx.download(do, (k, chw))
        for j in range(k):
            ctx.rows_mean_dev(dt, n_rows, chw, rows[j, :kept[j]], d1)
            assert np.array_equal(faces[j].view(np.uint32), ctx.download(d1, (chw,)).view(np.uint32)), j
        assert not faces[0].any()
        assert np.array_equal(faces[1], table[rows[1, 0]] / np.float32(1))
        # entries outside the table are skipped, not read
        bad = rows.copy(); bad[2, 5] = n_rows; bad[2, 9] = -3; bad[3, 0] = 2 ** 40
        ctx.upload(bad, dr)
        ctx.cluster_faces_dev(dt, n_rows, chw, dr, dk, k, m, do)
        got = ctx.download(do, (k, chw))
        acc = np.zeros(chw, np.float32)
        for r in bad[2, :71]:
            if 0 <= r < n_rows:
                acc = acc + table[r]
        assert np.array_equal(got[2], acc / np.float32(71)) and np.isfinite(got).all()


@pytest.mark.parametrize("closest", [False, True])
def test_create_cluster_images_dev_with_a_device_table(ctx, closest):
    from ganrev import apply_r, synth
    from ganrev.nn_utils import DeviceTensor
    N, nd = 600, 32
    attrs = synth.normal((N, nd), 81)
    attrs[:200] += 1.0
    images = synth.uniform((N, 1, 8, 8), 82, 0, 1)
    di, da = DeviceTensor(ctx, images.shape), DeviceTensor(ctx, attrs.shape)
    ctx.upload(images, di.ptr); ctx.upload(attrs, da.ptr)
    try:
        res = []
        for table in (attrs, da):
            cent, counts, clusters, faces = apply_r.createClusterImagesDev(20, 15, 71, di, table, seed=3, closest=closest)
            res.append((cent, counts, clusters, faces.numpy()))
            faces.free()
    finally:
        di.free(); da.free()
    (c0, n0, l0, f0), (c1, n1, l1, f1) = res
    assert np.array_equal(c0, c1) and np.array_equal(n0, n1) and c0.dtype == c1.dtype and n0.dtype == n1.dtype
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32)) and f0.shape == f1.shape
    assert l0 == l1 and [[(type(r), type(v)) for r, v in c] for c in l0] == [[(type(r), type(v)) for r, v in c] for c in l1]
    assert sum(len(c) for c in l0) > 0
