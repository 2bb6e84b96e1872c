"""-m gpu: the exact L2 nearest-neighbour search (gr_l2_nearest_host / _dev, neighbours.hip) against the oracle, bit for bit, and
sample.lua's compute on top of it (nn_utils.sortImagesByPrediction, ganrev.sample).

Reference: oracle.l2_distance_rows(table, broadcast query) per query - torch.dist's sequential fp64 sum of fp32 squares, the
convention the search promises - then the (dist, row) order by np.lexsort, NaN last.  Distances compare by their bits."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIRECT_ROWS = 4096          # neighbours.hip L2_DIRECT_ROWS: up to here the exact path is taken outright
CAND_MAX = 256              # neighbours.hip L2_CAND_MAX


def oracle_nearest(oracle, table, queries, k, workers=16):
    """k nearest rows per query by (dist, row), NaN last; the queries on a pool of threads, the table in slices of rows (each
    slice's broadcast copy stays small); every row's distance is computed on its own, so neither split changes a bit."""
    from concurrent.futures import ThreadPoolExecutor
    table = np.ascontiguousarray(table, np.float32).reshape(len(table), -1)
    queries = np.ascontiguousarray(queries, np.float32).reshape(-1, table.shape[1])
    oracle.lib()

    def one(q):
        oracle.set_threads(1)
        dist = np.empty(len(table), np.float64)
        for s in range(0, len(table), 8192):
            part = table[s:s + 8192]
            dist[s:s + len(part)] = oracle.l2_distance_rows(part, np.broadcast_to(q, part.shape))
        order = np.lexsort((np.arange(len(table)), dist))[:k]
        return order, dist[order]
    with ThreadPoolExecutor(max_workers=max(1, min(workers, os.cpu_count() or 1, len(queries)))) as ex:
        res = list(ex.map(one, queries))
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def assert_same(idx, dist, ridx, rdist, what=""):
    assert np.array_equal(idx, ridx), f"{what}: indices differ at {np.argwhere(idx != ridx)[:5].tolist()}"
    assert np.array_equal(dist.view(np.int64), rdist.view(np.int64)), f"{what}: distances differ in their bits"


def kernels_of(ctx, fn):
    ctx.set_timing(2)
    try:
        out = fn()
        names = {r["kernel"] for r in ctx.kernel_times()}
    finally:
        ctx.set_timing(0)
    return out, names


def rand_table(n, d, seed):
    return np.random.default_rng(seed).random((n, d), dtype=np.float32)


# (n, d, q, k): together every d of {1, 3, 100, 1024, 3072, 12288}, n of {1, 7, 4097, 131071, 200000 at d = 1024},
# q of {1, 5, 16, 17, 64}, k of {1, 8, 128, k = n}
SWEEP = [
    (1, 1, 1, 1), (7, 3, 5, 7), (7, 100, 17, 1), (4097, 3, 64, 8), (4097, 1024, 16, 128), (4097, 100, 64, 128),
    (131071, 100, 5, 8), (200000, 1024, 16, 1), (20000, 3072, 17, 8), (6000, 12288, 5, 8), (3000, 1, 5, 128),
]


@pytest.mark.parametrize("n,d,q,k", SWEEP, ids=[f"n{n}_d{d}_q{q}_k{k}" for n, d, q, k in SWEEP])
def test_sweep_vs_oracle(ctx, oracle, n, d, q, k):
    x = rand_table(n, d, n + d)
    qs = np.random.default_rng(q * 7 + k).random((q, d), dtype=np.float32)
    (idx, dist), names = kernels_of(ctx, lambda: ctx.l2_nearest(x, qs, k))
    ridx, rdist = oracle_nearest(oracle, x, qs, k)
    assert_same(idx, dist, ridx, rdist, "host")
    xd = ctx.upload(x)
    try:
        idx2, dist2 = ctx.l2_nearest(None, qs, k, table_dev=xd, n=n, d=d)
    finally:
        ctx.free(xd)
    assert_same(idx2, dist2, idx, dist, "dev vs host")
    if n > DIRECT_ROWS:
        assert "l2_approx_kernel" in names and "l2_select_kernel" in names and "l2_exact_kernel" not in names, names
    else:
        assert "l2_exact_kernel" in names and "l2_approx_kernel" not in names, names


def test_planted_copies(ctx, oracle):
    x = rand_table(50000, 1024, 11)
    x[30000] = x[10]; x[40000] = x[10]
    qs = x[[10, 20000, 49999]].copy()
    idx, dist = ctx.l2_nearest(x, qs, 4)
    assert idx[0, :3].tolist() == [10, 30000, 40000] and (dist[0, :3] == 0).all()
    assert idx[1, 0] == 20000 and idx[2, 0] == 49999 and dist[1, 0] == 0 and dist[2, 0] == 0
    assert_same(idx, dist, *oracle_nearest(oracle, x, qs, 4))


def test_near_ties_inside_the_window(ctx, oracle):
    rng = np.random.default_rng(5)
    x = rand_table(20000, 1024, 12)
    base = x[300].copy()
    one = base.copy(); one[17] = np.nextafter(one[17], np.float32(2))
    many = base.copy(); many[::3] = np.nextafter(many[::3], np.float32(2))
    x[100] = one; x[200] = many; x[5000] = base
    qs = np.stack([base, base + rng.normal(0, 1e-3, base.shape).astype(np.float32)])
    (idx, dist), names = kernels_of(ctx, lambda: ctx.l2_nearest(x, qs, 8))
    assert_same(idx, dist, *oracle_nearest(oracle, x, qs, 8))
    assert idx[0, :2].tolist() == [300, 5000]
    assert "l2_exact_kernel" not in names, names


def test_overflow_takes_the_exact_path(ctx, oracle):
    rng = np.random.default_rng(7)
    x = rand_table(20000, 100, 13)
    rows = rng.choice(np.arange(1, 20000), 300, replace=False)
    x[rows] = x[0]
    qs = (x[0] + rng.normal(0, 1e-2, 100)).astype(np.float32)[None]
    (idx, dist), names = kernels_of(ctx, lambda: ctx.l2_nearest(x, qs, 8))
    assert "l2_exact_kernel" in names and "l2_approx_kernel" in names, names       # the fast path ran, overflowed, the exact one decided
    assert_same(idx, dist, *oracle_nearest(oracle, x, qs, 8))
    assert idx[0].tolist() == sorted([0] + rows.tolist())[:8]

    c = np.full((10000, 64), 0.25, np.float32)
    q = np.full((2, 64), 0.5, np.float32)
    (idx, dist), names = kernels_of(ctx, lambda: ctx.l2_nearest(c, q, 128))
    assert "l2_exact_kernel" in names, names
    assert (idx == np.arange(128)).all()
    assert (dist == np.sqrt(64 * 0.0625)).all()


@pytest.mark.parametrize("scale", [2.0 ** -70, 2.0 ** 62, "nan"])
def test_range(ctx, oracle, scale):
    rng = np.random.default_rng(9)
    x = rng.normal(0, 1, (10000, 256)).astype(np.float32)
    qs = rng.normal(0, 1, (3, 256)).astype(np.float32)
    if scale == "nan":
        x[1, 7] = np.nan; x[50, 0] = np.nan
        k = 8
    else:
        x *= np.float32(scale); qs *= np.float32(scale)
        k = 16
    idx, dist = ctx.l2_nearest(x, qs, k)
    assert_same(idx, dist, *oracle_nearest(oracle, x, qs, k))
    if scale == 2.0 ** 62:
        assert np.isinf(oracle_nearest(oracle, x, qs[:1], 10000)[1]).any()      # some squares overflow to +inf
    if scale == "nan":                           # a NaN distance orders after everything, +inf included: the last places of a full ranking
        t = x[:128].copy(); t[3, 0] = np.inf
        idx, dist = ctx.l2_nearest(t, qs[:1], 128)
        assert_same(idx, dist, *oracle_nearest(oracle, t, qs[:1], 128))
        assert idx[0, -3:].tolist() == [3, 1, 50] and np.isinf(dist[0, -3]) and np.isnan(dist[0, -2:]).all()


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.h
    x = rand_table(200, 8, 1); q = rand_table(2, 8, 2)
    idx = np.empty(2 * 200, np.int64); dist = np.empty(2 * 200, np.float64)
    P = lambda a: C.c_void_p(a.ctypes.data)          # noqa: E731
    calls = [
        ((None, 200, 8, P(q), 2, 1, P(idx), P(dist)), -1), ((P(x), 200, 8, None, 2, 1, P(idx), P(dist)), -1),
        ((P(x), 200, 8, P(q), 2, 1, None, P(dist)), -1), ((P(x), 200, 8, P(q), 2, 1, P(idx), None), -1),
        ((P(x), 0, 8, P(q), 2, 1, P(idx), P(dist)), -1), ((P(x), -3, 8, P(q), 2, 1, P(idx), P(dist)), -1),
        ((P(x), 200, 0, P(q), 2, 1, P(idx), P(dist)), -1), ((P(x), 200, 65537, P(q), 2, 1, P(idx), P(dist)), -1),
        ((P(x), 200, 8, P(q), 0, 1, P(idx), P(dist)), -1), ((P(x), 200, 8, P(q), 65, 1, P(idx), P(dist)), -1),
        ((P(x), 200, 8, P(q), 2, 0, P(idx), P(dist)), -1), ((P(x), 200, 8, P(q), 2, 201, P(idx), P(dist)), -1),
        ((P(x), 200, 8, P(q), 2, 129, P(idx), P(dist)), -2),
    ]
    for args, want in calls:
        assert lib.gr_l2_nearest_host(h, *args) == want, args
        assert lib.gr_l2_nearest_dev(h, *args) == want, args
        got = ctx.l2_nearest(x, q, 3)
        assert got[0].shape == (2, 3)
    assert lib.gr_l2_nearest_host(None, P(x), 200, 8, P(q), 2, 1, P(idx), P(dist)) == -1


def test_sort_images_by_prediction_d2(ctx):
    from ganrev import models, nn_utils, synth
    dims = (3, 32, 32)
    D = models.create_D2(dims, seed=3); synth.init_params(D, 19)
    D.evaluate()
    images = synth.uniform((40,) + dims, 5, 0, 1)
    pred = nn_utils.forwardBatched(D, images, 16).reshape(40, -1)[:, 0]
    for asc in (True, False):
        for m in (7, 100):
            got_i, got_p = nn_utils.sortImagesByPrediction(D, images, asc, m, 16)
            order = np.argsort(pred if asc else -pred, kind="stable")[:min(m, 40)]
            assert np.array_equal(got_p, pred[order]) and np.array_equal(got_i, images[order])
            assert len(got_i) == min(m, 40)


def test_sample_end_to_end(ctx, tmp_path):
    from ganrev import models, nn_utils, sample, synth, t7
    dims = (1, 32, 32)
    G = models.create_G(dims, 32, True, 4); synth.init_params(G, 4)
    D = models.create_D(dims, True, 5); synth.init_params(D, 5)
    t7.save_checkpoint(str(tmp_path / "adversarial.net"), G=G, D=D, opt={"width": 32, "height": 32, "colorSpace": "y"})
    argv = ["--save", str(tmp_path), "--colorSpace", "y", "--writeTo", str(tmp_path / "out"), "--seed", "3"]
    opt = sample.parse(argv)
    G2, D2 = sample.loadModels(opt)
    images = nn_utils.createImages(G2, 1024, opt.noiseDim, opt.batchSize, opt.noiseMethod, sample.noise_seed(opt, 1))
    best, _ = nn_utils.sortImagesByPrediction(D2, images, False, 64, opt.batchSize)
    data = np.random.default_rng(0).random((5000,) + dims, dtype=np.float32)
    planted = [4321, 17, 2500]
    for r, b in zip(planted, best[:3]):
        data[r] = b
    np.save(tmp_path / "data.npy", data)
    paths = sample.main(argv + ["--data", str(tmp_path / "data.npy"), "--neighbours", "--runs", "1"])
    z = np.load(paths[0])
    assert z["best"].shape == (64,) + dims and z["worst"].shape == (64,) + dims and z["random"].shape == (64,) + dims
    assert (np.diff(z["best_pred"]) <= 0).all() and (np.diff(z["worst_pred"]) >= 0).all()
    assert z["neighbour_idx"].shape == (16,) and z["neighbour_dist"].shape == (16,) and z["neighbours"].shape == (16,) + dims
    assert z["neighbour_idx"][:3].tolist() == planted and (z["neighbour_dist"][:3] == 0).all()
    assert np.array_equal(z["neighbours"], data[z["neighbour_idx"]])
