"""-m gpu: search by example - the cosine top-k search with needles that are vectors of their own (gr_cosine_topk_queries_*) on every
dispatch path of search.hip.

Two references:
  * a needle that IS a table row, bit for bit, must return what the row-index search of that row returns: indices, score bits, reruns and the
    kernels that ran (the core invariant: everything behind the needle fetch sees the same bits);
  * needles from outside the table against append-and-filter on the unchanged oracle (search_queries_oracle.append_and_filter), bit for bit.

The paths and their kernels are those of tests/test_gpu_search_paths.py, restated here (search.hip, launch_cosine_topk).

The zero needle.  Its score is 0 against every row, so ALL N rows tie at the k-th place: no sample bound or approximate cut can separate
them, every candidate list overflows and the call reruns on the plain path - on the small and the filter path one rerun is what the design
gives, as for the batched path's range rule.  The outside-needle cases therefore run twice: without the zero needle (search_reruns must not
move: the approximate path is what was checked) and with it (exact; one rerun on an approximate path, none on the plain path)."""
import numpy as np
import pytest

from search_queries_oracle import append_and_filter

pytestmark = pytest.mark.gpu

FILTER_MIN_ROWS = 1 << 17
SAMPLE_ROWS = 16384
N17 = 1 << 17
PATH_KERNELS = {
    "small": {"cos_approx_kernel (sample + bound)", "cos_approx_kernel", "small_select_kernel"},
    "batched": {"cos_mfma_kernel (sample)", "batched_tau_wave_kernel", "cos_mfma_kernel", "batched_select_kernel"},
    "filter": {"cos_keys_kernel (sample)", "topk_select_kernel (bound)", "cos_keys_kernel", "topk_select_kernel"},
    "plain": {"cos_keys_kernel", "topk_pass_kernel"},
}


def search_path(N, d, Q, k):
    """launch_cosine_topk's predicates (the same for both needle sources)"""
    k = min(k, N)
    filt = N >= FILTER_MIN_ROWS and k * 8 <= SAMPLE_ROWS and k <= 1024
    if filt and 1 <= Q <= 8 and d % 4 == 0 and d // 4 in (8, 16, 25, 32) and k <= 128 and N * d * 4 < 0x7FFFF000:
        return "small"
    if filt and 32 <= Q <= 2048 and d <= 128 and k <= 128 and N >= 2 * 65536:
        return "batched"
    return "filter" if filt else "plain"


# ---------------------------------------------------------------- tables: standard normal rows; rows 0, 1000 and N - 1 have an exact duplicate further
# down (a score tie resolved by index); row 3 is zero except on the batched path's tables (one zero row sends that path to its rerun)
def _normal(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def _dups(N):
    return {0: N // 2 + 1, 1000: N // 3, N - 1: 2 * N // 3}


def _featured(N, d, seed, zero=True):
    emb = _normal((N, d), seed)
    for src, dst in _dups(N).items():
        emb[dst] = emb[src]
    if zero:
        emb[3] = 0.0
    return emb


def _hostile(N, d, seed):
    """Built against the sample (rows i * (N // 16384)): every sampled row is random, every other row lies within 1e-3 of one vector v - for a
    needle near v nearly every row passes the sample's threshold.  Row 1000 is v itself."""
    emb = _normal((N, d), seed)
    h = emb[1000][None, :] + np.float32(1e-3) * _normal((N, d), seed + 1)
    stride = N // SAMPLE_ROWS
    h[::stride] = emb[::stride]
    h[1000] = emb[1000]
    return h


TABLES = {
    "p30": lambda: _featured(4097, 30, 301),
    "n100": lambda: _featured(N17, 100, 1001),
    "n32": lambda: _featured(N17, 32, 321),
    "r64": lambda: _featured(140_001, 64, 641),
    "b64": lambda: _featured(N17, 64, 642, zero=False),
    "b113": lambda: _featured(N17, 113, 1131, zero=False),
    "hostile64": lambda: _hostile(262_144, 64, 643),
}
_TABLE_CACHE, _REF_CACHE = {}, {}


def table(name):
    if name not in _TABLE_CACHE:
        _TABLE_CACHE[name] = np.ascontiguousarray(TABLES[name](), dtype=np.float32)
    return _TABLE_CACHE[name]


def needle_rows(Q, N):
    """the anchors of test_gpu_search_paths.needles_for: row 0, row N - 1, a duplicated row (1000) and the same row twice, then a spread"""
    if Q == 1:
        return np.array([N - 1], dtype=np.int64)
    head = [0, 1000, N - 1, 1000]
    return np.array((head + [(i * 7919 + 11) % N for i in range(max(0, Q - 4))])[:Q], dtype=np.int64)


def outside_needles(emb, Q, seed, zero):
    """Q vectors that are not searched as rows: a row plus a small perturbation, a row times 2^3, a copy of a duplicated row (ties on index), fresh
    vectors of the table's distribution and - last, when asked for - a zero needle"""
    N, d = emb.shape
    nd = _normal((Q, d), seed)
    nd[0] = emb[1000] + np.float32(1e-2) * nd[0]
    if Q > 1:
        nd[1] = emb[N - 1] * np.float32(8.0)
    if Q > 2:
        nd[2] = emb[0]
    if zero and Q > 3:
        nd[Q - 1] = 0.0
    return np.ascontiguousarray(nd)


def reference(oracle, tname, key, needles, k, accf):
    if (tname, key, k, accf) not in _REF_CACHE:
        _REF_CACHE[(tname, key, k, accf)] = append_and_filter(oracle, table(tname), needles, k, accf)
    return _REF_CACHE[(tname, key, k, accf)]


def assert_exact(name, idx, sc, ridx, rsc):
    assert idx.shape == ridx.shape and sc.shape == rsc.shape, (name, idx.shape, ridx.shape)
    assert sc.dtype == rsc.dtype == np.float32
    bad = np.nonzero(~(idx == ridx).all(axis=1) | ~(sc.view(np.uint32) == rsc.view(np.uint32)).all(axis=1))[0]      # score BITS: -0 is not +0
    assert bad.size == 0, (f"{name}: needles {bad[:8].tolist()} differ from the reference; first: got {idx[bad[0]][:8].tolist()} "
                           f"{sc[bad[0]][:8].tolist()}, want {ridx[bad[0]][:8].tolist()} {rsc[bad[0]][:8].tolist()}")
    assert np.all(sc[:, :-1] >= sc[:, 1:]), f"{name}: scores must be sorted descending"
    tie = sc[:, :-1] == sc[:, 1:]
    assert np.all(idx[:, :-1][tie] < idx[:, 1:][tie]), f"{name}: ties are ordered by ascending index"


def timed_names(c, fn):
    c.set_timing(2)
    try:
        res = fn()
        names = {t["kernel"] for t in c.kernel_times()}
    finally:
        c.set_timing(0)
    return res, names - {"range_guard_fallback"}


# ---------------------------------------------------------------- 1. rows as queries
ROW_CASES = [  # (name, table, Q, k, path)
    ("plain_4097x30_q9_k50", "p30", 9, 50, "plain"),
    ("filter_d100_q13_k50_dc20", "n100", 13, 50, "filter"),
    ("small_d100_q5_k50", "n100", 5, 50, "small"),
    ("small_d32_q1_k1", "n32", 1, 1, "small"),
    ("small_d64_q8_k128_ragged", "r64", 8, 128, "small"),
    ("batched_d64_q40_k50", "b64", 40, 50, "batched"),
    ("batched_d113_q32_k128", "b113", 32, 128, "batched"),
]


@pytest.mark.parametrize("accf", [False, True], ids=["acc64", "acc32"])
@pytest.mark.parametrize("case", ROW_CASES, ids=[c[0] for c in ROW_CASES])
def test_rows_as_queries_equal_the_row_index_search(ctx, case, accf):
    """cosine_topk_queries(emb, emb[rows]) == cosine_topk(emb, rows): indices, score bits and reruns, on the kernels of the path the shape selects"""
    name, tname, Q, k, path = case
    emb = table(tname)
    N, d = emb.shape
    assert search_path(N, d, Q, k) == path
    rows = needle_rows(Q, N)
    r0 = ctx.search_reruns()
    ridx, rsc = ctx.cosine_topk(emb, rows, k, accumulate_in_float=accf)
    r1 = ctx.search_reruns()
    idx, sc = ctx.cosine_topk_queries(emb, emb[rows], k, accumulate_in_float=accf)
    r2 = ctx.search_reruns()
    print(f"{name}: row-index reruns {r1 - r0}, by-example reruns {r2 - r1}")
    assert_exact(name, idx, sc, ridx, rsc)
    assert r2 - r1 == r1 - r0 == 0, f"{name}: reruns {r1 - r0} (rows) / {r2 - r1} (vectors): the approximate path was not what ran"
    (tidx, tsc), names = timed_names(ctx, lambda: ctx.cosine_topk_queries(emb, emb[rows], k, accumulate_in_float=accf))
    assert names == PATH_KERNELS[path], f"{name}: launched {sorted(names)}, the {path} path is {sorted(PATH_KERNELS[path])}"
    assert np.array_equal(tidx, idx) and np.array_equal(tsc.view(np.uint32), sc.view(np.uint32))


# ---------------------------------------------------------------- 2. outside needles against the oracle
OUTSIDE_CASES = [  # (name, table, Q, k, accf, path, zero needle in the second run)
    ("plain_4097x30_q9_k50_acc32", "p30", 9, 50, True, "plain", True),
    ("filter_d100_q13_k50", "n100", 13, 50, False, "filter", True),
    ("small_d100_q5_k50", "n100", 5, 50, False, "small", True),
    ("batched_d64_q40_k50_acc32", "b64", 40, 50, True, "batched", False),
]


@pytest.mark.parametrize("case", OUTSIDE_CASES, ids=[c[0] for c in OUTSIDE_CASES])
def test_outside_needles_bit_exact(ctx, oracle, case):
    """Needles that are not table rows equal append-and-filter on the oracle bit for bit; without the zero needle nothing reruns (see the head
    of this file for the zero needle)."""
    name, tname, Q, k, accf, path, zero = case
    emb = table(tname)
    N, d = emb.shape
    needles = outside_needles(emb, Q, 77, zero)
    ridx, rsc = reference(oracle, tname, ("outside", Q, zero), needles, k, accf)
    nz = Q - 1 if zero else Q                                   # the needles in front of the zero needle
    assert search_path(N, d, nz, k) == search_path(N, d, Q, k) == path
    r0 = ctx.search_reruns()
    (idx, sc), names = timed_names(ctx, lambda: ctx.cosine_topk_queries(emb, needles[:nz], k, accumulate_in_float=accf))
    reruns = ctx.search_reruns() - r0
    print(f"{name}: {nz} needles, reruns {reruns}")
    assert_exact(name, idx, sc, ridx[:nz], rsc[:nz])
    assert reruns == 0, f"{name}: {reruns} reruns on a random table: pick another seed, the approximate path must be what is checked"
    assert names == PATH_KERNELS[path], (name, sorted(names))
    if zero:
        r0 = ctx.search_reruns()
        idx, sc = ctx.cosine_topk_queries(emb, needles, k, accumulate_in_float=accf)
        reruns = ctx.search_reruns() - r0
        print(f"{name}: with the zero needle, reruns {reruns}")
        assert_exact(name + " (zero needle)", idx, sc, ridx, rsc)
        assert np.array_equal(idx[-1], np.arange(k)) and not sc[-1].any(), "a zero needle scores 0 everywhere: rows 0 .. k - 1"
        assert reruns == (0 if path == "plain" else 1), f"{name}: {reruns} reruns with the zero needle"


# ---------------------------------------------------------------- 3. overflow rerun
def test_overflow_rerun_with_outside_needles(ctx, oracle):
    """A table built against the sample, needles near the vector its rows crowd around: the small path's lists overflow, exactly one rerun, exact"""
    emb = table("hostile64")
    N, d = emb.shape
    needles = _normal((5, d), 78)
    needles[1] = emb[1000] + np.float32(1e-4) * needles[1]
    needles[2] = emb[1000] * np.float32(8.0)
    needles[4] = emb[1000]
    assert search_path(N, d, 5, 50) == "small"
    ridx, rsc = reference(oracle, "hostile64", "hostile", needles, 50, False)
    r0 = ctx.search_reruns()
    idx, sc = ctx.cosine_topk_queries(emb, needles, 50)
    reruns = ctx.search_reruns() - r0
    assert_exact("hostile64", idx, sc, ridx, rsc)
    assert reruns == 1, reruns


# ---------------------------------------------------------------- 4. the batched path's range rule
def test_batched_zero_needle_reruns_exact(ctx, oracle):
    """One zero needle among 31 normal ones: its squared norm is outside what the fp16 candidate pass carries, its threshold is -inf, every
    list overflows: one rerun, exact result"""
    emb = table("b64")
    N, d = emb.shape
    needles = outside_needles(emb, 32, 79, True)
    assert not needles[-1].any() and search_path(N, d, 32, 50) == "batched"
    ridx, rsc = reference(oracle, "b64", "zero32", needles, 50, False)
    r0 = ctx.search_reruns()
    idx, sc = ctx.cosine_topk_queries(emb, needles, 50)
    reruns = ctx.search_reruns() - r0
    assert_exact("batched zero needle", idx, sc, ridx, rsc)
    assert reruns == 1, reruns


def test_batched_needle_beyond_fp16_reruns_exact(ctx, oracle):
    """One needle = a row times 2^17 among 31 normal ones: finite in fp32, but its elements overflow fp16 - the staged image holds inf, the
    candidate pass's dot products are inf - inf = NaN, which pass no threshold, not even -inf: its lists stay EMPTY instead of overflowing.
    The needle's own norm (outside [2^-10, 65504^2]) must send the call to its rerun: one rerun, exact result."""
    emb = table("b64")
    N, d = emb.shape
    needles = outside_needles(emb, 32, 82, False)
    needles[5] = emb[777] * np.float32(2.0 ** 17)
    assert np.abs(needles[5]).max() > 65504 and np.isfinite(needles[5].astype(np.float64) ** 2).all() and search_path(N, d, 32, 50) == "batched"
    ridx, rsc = reference(oracle, "b64", "big32", needles, 50, False)
    assert ridx[5][0] == 777
    r0 = ctx.search_reruns()
    idx, sc = ctx.cosine_topk_queries(emb, needles, 50)
    reruns = ctx.search_reruns() - r0
    assert_exact("batched needle beyond fp16", idx, sc, ridx, rsc)
    assert reruns == 1, reruns


# ---------------------------------------------------------------- 5. state across calls
def test_small_path_state_across_needle_sources(oracle):
    """The small path's context state (arrival counter, histogram, completion words, sequence number) is shared by both needle sources: on one
    fresh context a row search, a search by example, the row search again, a search by example at another d.  Every call exact; first == third."""
    import ganrev._lib as L
    from helpers import oracle_topk_parallel
    emb, emb32 = table("n100"), table("n32")
    rows = needle_rows(5, N17)
    nd100, nd32 = outside_needles(emb, 5, 77, True)[:4], outside_needles(emb32, 3, 80, False)
    if ("n100", "rows5") not in _REF_CACHE:
        _REF_CACHE[("n100", "rows5")] = oracle_topk_parallel(oracle, emb, rows, 50)
    row_ref = _REF_CACHE[("n100", "rows5")]
    ref100 = reference(oracle, "n100", ("outside", 5, True), outside_needles(emb, 5, 77, True), 50, False)     # (shared with the small case above)
    ref32 = reference(oracle, "n32", "seq32", nd32, 50, False)
    c = L.Context(0)
    try:
        r0 = c.search_reruns()
        a = c.cosine_topk(emb, rows, 50)
        assert_exact("call 0 (rows)", a[0], a[1], *row_ref)
        b = c.cosine_topk_queries(emb, nd100, 50)
        assert_exact("call 1 (vectors)", b[0], b[1], ref100[0][:4], ref100[1][:4])
        a2 = c.cosine_topk(emb, rows, 50)
        assert_exact("call 2 (rows)", a2[0], a2[1], *row_ref)
        assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1])
        e = c.cosine_topk_queries(emb32, nd32, 50)
        assert_exact("call 3 (vectors, d = 32)", e[0], e[1], *ref32)
        assert c.search_reruns() == r0
    finally:
        c.close()


# ---------------------------------------------------------------- 6. arguments
def test_arguments(ctx, oracle):
    import ctypes as C
    import ganrev._lib as L
    emb = table("p30")
    N, d = emb.shape
    needles = outside_needles(emb, 3, 81, False)
    idx = np.empty((3, 1025), np.int64); sc = np.empty((3, 1025), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda fn, q_ptr, q, k: fn(ctx.h, p(emb), N, d, q_ptr, q, k, p(idx), p(sc), 0)
    for fn in (ctx.lib.gr_cosine_topk_queries_host, ctx.lib.gr_cosine_topk_queries_dev):
        assert call(fn, None, 3, 5) == -1, "null queries: GR_ERR_INVALID"
        assert call(fn, p(needles), 0, 5) == -1, "q = 0: GR_ERR_INVALID"
        assert call(fn, p(needles), 3, 0) == -1, "k = 0: GR_ERR_INVALID"
    assert call(ctx.lib.gr_cosine_topk_queries_host, p(needles), 3, 1025) == -2, "k = 1025: GR_ERR_UNSUPPORTED"
    with pytest.raises(L.GanrevError):
        ctx.cosine_topk_queries(emb, needles, 1025)
    # k > n is clamped
    small = emb[:7]
    i7, s7 = ctx.cosine_topk_queries(small, needles, 50)
    r7 = append_and_filter(oracle, small, needles, 50)
    assert i7.shape == (3, 7)
    assert_exact("k > n", i7, s7, *r7)
    # a device table with host needles, and with device needles, equals all-host
    hi, hs = ctx.cosine_topk_queries(emb, needles, 20)
    demb, dq = ctx.upload(emb), ctx.upload(needles)
    try:
        di, ds = ctx.cosine_topk_queries(None, needles, 20, emb_dev=demb, n=N, d=d)
        qi, qs = ctx.cosine_topk_queries(None, None, 20, emb_dev=demb, n=N, d=d, queries_dev=dq, q=3)
    finally:
        ctx.free(demb); ctx.free(dq)
    assert np.array_equal(hi, di) and np.array_equal(hs, ds) and np.array_equal(hi, qi) and np.array_equal(hs, qs)


def test_needle_array_that_is_not_16_byte_aligned(ctx, oracle):
    """The small path fetches outside needles as float4s: a needle array 4 bytes off takes the filter path instead (results through the
    same pinned block, one stream wait) - exact, no rerun, the filter path's kernels"""
    emb = table("n100")
    N, d = emb.shape
    needles = outside_needles(emb, 5, 77, True)[:4]
    ref = reference(oracle, "n100", ("outside", 5, True), outside_needles(emb, 5, 77, True), 50, False)
    assert search_path(N, d, 4, 50) == "small"
    demb, buf = ctx.upload(emb), ctx.malloc(4 * (needles.size + 4))
    try:
        ctx.upload(needles, buf + 4)
        r0 = ctx.search_reruns()
        (idx, sc), names = timed_names(ctx, lambda: ctx.cosine_topk_queries(None, None, 50, emb_dev=demb, n=N, d=d, queries_dev=buf + 4, q=4))
        assert ctx.search_reruns() == r0
        ctx.upload(needles, buf)
        (aidx, asc), anames = timed_names(ctx, lambda: ctx.cosine_topk_queries(None, None, 50, emb_dev=demb, n=N, d=d, queries_dev=buf, q=4))
    finally:
        ctx.free(demb); ctx.free(buf)
    assert_exact("needles 4 bytes off", idx, sc, ref[0][:4], ref[1][:4])
    assert_exact("needles aligned", aidx, asc, ref[0][:4], ref[1][:4])
    assert names == PATH_KERNELS["filter"] and anames == PATH_KERNELS["small"], (sorted(names), sorted(anames))


def test_sharded_search_of_a_device_resident_shard(ctx, oracle):
    """parallel.sharded_cosine_topk_queries with Context.cosine_topk_queries as the local search (parallel.context_topk_queries): a shard that
    is a DeviceTensor is searched where it lies and gives the host shard's lists, with the shard's row offset added"""
    from ganrev.nn_utils import DeviceTensor
    from ganrev.parallel import LocalCommunicator, context_topk_queries, sharded_cosine_topk_queries
    emb = table("n32")
    nd32 = outside_needles(emb, 3, 80, False)
    ref = reference(oracle, "n32", "seq32", nd32, 50, False)
    local = context_topk_queries(ctx)
    hi, hs = sharded_cosine_topk_queries(local, emb, 1000, nd32, 50, LocalCommunicator())
    shard = DeviceTensor(ctx, emb.shape)
    try:
        ctx.upload(emb, shard.ptr)
        di, ds = sharded_cosine_topk_queries(local, shard, 1000, nd32, 50, LocalCommunicator())
    finally:
        shard.free()
    assert_exact("host shard", hi - 1000, hs, *ref)
    assert_exact("device shard", di - 1000, ds, *ref)
