"""-m gpu: every dispatch path of the cosine top-k search (search.hip, launch_cosine_topk) against the oracle, bit for bit.

The search promises indices AND scores equal to oracle.cosine_topk, ties included (score descending, then row ascending).  To keep that
promise at speed, launch_cosine_topk picks one of four paths from (N, d, Q, k), and inside each path it picks templates again:

  small     <= 8 needles, d in {32, 64, 100, 128}: cos_approx_kernel<D4, NQ, MODE> (fp32 approximate scores, margin eps2), small_select_kernel
  batched   32..2048 needles, d <= 128, k <= 128: cos_mfma_kernel<MODE, NK> (fp16 MFMA approximate scores, margin 2 GR_BERR), batched_select_kernel
  filter    N >= 2^17, k <= 1024, not one of the above: cos_keys_kernel<ACCF, MODE, NQ, DC> on a sample for a bound, then on every row
  plain     everything else, and every rerun: cos_keys_kernel<ACCF, 0, NQ, DC> on every row, topk_pass_kernel

The three approximate paths end in an exact re-score; when their candidate lists overflow, the call reruns on the plain path and counts one
search_reruns().  search_path() below restates the dispatch predicates; every case names the path it expects, the coverage test checks that
the case table reaches every leaf, and each case's timed run checks from kernel_times() that the library took the path the mirror predicts.

Out of scope: non-finite inputs (rows with inf or NaN, or elements so large that x * x overflows fp32).  Their scores are NaN, and the
reference's table.sort has no defined order for NaN; the device key (orderable) and the oracle's qsort comparator disagree on it.  Defining
that order is a separate decision.  Scores compare with == (np.array_equal), so -0 equals +0: orderable() folds -0 into +0 so that equal
scores tie by index as in the oracle's comparator, and a score the oracle returns as -0 (range_*_2p60: every score underflows) comes back
as +0.  The sign of a zero score is the one bit these tests do not compare.

Cost: the oracle sorts all N rows per needle, so references are computed once per (table, accumulate_in_float) for the largest k any case
asks of that table (top-k at a smaller k is a prefix: the order is total), on a pool of threads (helpers.oracle_topk_parallel)."""
import dataclasses

import numpy as np
import pytest

from helpers import oracle_topk_parallel

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- the dispatch, restated (gan-reverser_amd/csrc/search.hip)
QG = 8                      # :31  needles per cos_keys_kernel pass
CHUNK = 2048                # :33  keys per top-k workgroup
FILTER_MIN_ROWS = 1 << 17   # :34
SAMPLE_ROWS = 16384         # :35  the filter path's sample
BATCH_MIN_Q = 32            # :321
AQ_MAX = 8                  # :322 needles of the small path
BQ_MAX = 2048               # :324 needles of the batched path
BSAMPLE_ROWS = 65536        # :325 the batched path's sample
BD_MAX = 128                # :327
SMALL_K_MAX = 128           # :1023 (cosine_topk_small_path)
BATCH_K_MAX = 128           # :1287 (launch_cosine_topk, batched branch)
SMALL_D4 = (8, 16, 25, 32)  # :1183 the cos_approx_kernel instantiations


def small_path_ok(N, d, Q, k):
    """cosine_topk_small_path (search.hip:1181)"""
    return 1 <= Q <= AQ_MAX and d % 4 == 0 and d // 4 in SMALL_D4 and N >= FILTER_MIN_ROWS and k <= SMALL_K_MAX and N * d * 4 < 0x7FFFF000


def search_path(N, d, Q, k):
    """The path launch_cosine_topk (search.hip:1244) takes on the first try of gr_cosine_topk_dev (ops.hip:173)."""
    k = min(k, N)
    filt = N >= FILTER_MIN_ROWS and k * 8 <= SAMPLE_ROWS and k <= CHUNK // 2                                  # :1258
    if filt and small_path_ok(N, d, Q, k):                                                                    # :1259
        return "small"
    if filt and BATCH_MIN_Q <= Q <= BQ_MAX and d <= BD_MAX and k <= BATCH_K_MAX and N >= 2 * BSAMPLE_ROWS:   # :1287
        return "batched"
    if filt:                                                                                                  # :1342
        return "filter"
    return "plain"                                                                                            # :1364


def approx_d4(d):
    """cos_approx_kernel's D4 (launch_approx, search.hip:1193)"""
    return d // 4


def approx_nq(Q):
    """cos_approx_kernel's NQ (launch_approx_nq, search.hip:1187)"""
    return 2 if Q <= 2 else (5 if Q <= 5 else 8)


def mfma_nk(d):
    """cos_mfma_kernel's NK (search.hip:1291)"""
    return 2 if d <= 32 else (4 if d <= 64 else (7 if d <= 112 else 8))


def keys_dc(d):
    """cos_keys_kernel's column chunk DC (launch_keys_nq, search.hip:1221)"""
    return 20 if d % 20 == 0 and d % 32 != 0 else 32


# kernel_times() names of each path (the KtScope labels in launch_cosine_topk); a rerun adds the plain path's
PATH_KERNELS = {
    "small": {"cos_approx_kernel (sample + bound)", "cos_approx_kernel", "small_select_kernel"},
    "batched": {"cos_mfma_kernel (sample)", "batched_tau_wave_kernel", "cos_mfma_kernel", "batched_select_kernel"},
    "filter": {"cos_keys_kernel (sample)", "topk_select_kernel (bound)", "cos_keys_kernel", "topk_select_kernel"},
    "plain": {"cos_keys_kernel", "topk_pass_kernel"},
}
K_MAX = {"small": SMALL_K_MAX, "batched": BATCH_K_MAX, "filter": CHUNK // 2, "plain": 1024}


# ---------------------------------------------------------------- tables
# Rows 0, 1000 and N - 1 are the anchor needles every case uses at least one of; each has an exact duplicate further down (a score tie
# resolved by index), and row 3 is zero (score 0 against everything) - except on the batched path's tables: ONE zero row is outside what the
# fp16 candidate pass can carry and sends the call to the plain path (test_gpu_parity's range-guard test; here the case "batched_zero_row").
POOL_SIZE = 140_001 * 128
_POOL = []


def _normal(N, d, seed):
    """N x d standard normal values: a window of one pool of synth.normal draws (the largest table's size), starting at a place the seed picks.
    Tables that share values this way are still different tables; the draws themselves would take most of this file's time."""
    from ganrev import synth
    if not _POOL:
        _POOL.append(synth.normal((POOL_SIZE,), 2026))
    off = (seed * 7919) % (POOL_SIZE - N * d + 1)
    return _POOL[0][off:off + N * d].reshape(N, d).copy()


def _dups(N):
    return {0: N // 2 + 1, 1000: N // 3, N - 1: 2 * N // 3}


def _featured(N, d, seed, zero=True):
    emb = _normal(N, d, seed)
    for src, dst in _dups(N).items():
        emb[dst] = emb[src]
    if zero:
        emb[3] = 0.0
    return emb


def _hostile(N, d, seed, needles):
    """Built against the sample: every sampled row (the small and filter paths sample rows i * (N // 16384)) is random, every other row lies
    within 1e-3 of needle 1000 - nearly every row passes the sample's threshold."""
    emb = _normal(N, d, seed)
    h = emb[1000][None, :] + np.float32(1e-3) * _normal(N, d, seed + 1)
    stride = N // SAMPLE_ROWS
    h[::stride] = emb[::stride]
    h[needles] = emb[needles]
    return h


def _near_tie(N, d, seed):
    """200 rows within 1e-3 (relative) of needle 1000, scattered over the table: their cosines with it lie within ~3e-7 of each other, a
    few fp32 steps below 1, many of them exactly equal - they straddle the k-th place of k = 100."""
    emb = _featured(N, d, seed)
    emb[NEAR_CLUSTER] = emb[1000][None, :] * (1 + np.float32(1e-3) * _normal(len(NEAR_CLUSTER), d, seed + 1))
    return emb


def _fp16_subnormal(N, d, seed):
    """In-range norms (|row| ~ 0.04, squared 1.6e-3 >= 2^-10), but all elements except one per row are ~3e-5: fp16 subnormals (< 6.1e-5).
    The large component sits at column row % d with a random sign.  Exact whether or not the fp16 MFMA flushes subnormal inputs."""
    from ganrev import synth
    emb = np.float32(3e-5) * _normal(N, d, seed)
    r = np.arange(N)
    emb[r, r % d] = np.where(synth.uniform((N,), seed + 1, 0, 1) < 0.5, -1.0, 1.0).astype(np.float32) * synth.uniform((N,), seed + 2, 0.035, 0.045)
    return emb


def _pixels(N, d, seed):
    """Gray 32 x 32 images (d = 1024, apply_r.lua:308-314's pixel-wise search), pixels in [0, 1): 64 random columns repeated over 16
    blocks of differently weighted columns (built in a fraction of the time 2^27 independent samples take)."""
    from ganrev import synth
    base = synth.uniform((N, 64), seed, 0, 1)
    w = synth.uniform((d,), seed + 1, 0.25, 1.0)
    emb = np.tile(base, (1, d // 64)) * w[None, :]
    for src, dst in _dups(N).items():
        emb[dst] = emb[src]
    emb[3] = 0.0
    return emb


N17 = 1 << 17
NEAR_CLUSTER = (np.arange(200, dtype=np.int64) * 661 + 13) % N17
HOSTILE_NEEDLES = np.array([0, 1000, 77_777, 262_143, 1000], dtype=np.int64)
TABLES = {         # name -> (N, d, builder)
    "n32": (N17, 32, lambda: _featured(N17, 32, 3201)),
    "n64": (N17, 64, lambda: _featured(N17, 64, 6401)),
    "n100": (N17, 100, lambda: _featured(N17, 100, 10001)),
    "n100r": (140_001, 100, lambda: _featured(140_001, 100, 10002)),
    "n128": (N17, 128, lambda: _featured(N17, 128, 12801)),
    "n128r": (140_001, 128, lambda: _featured(140_001, 128, 12802)),
    "near128": (N17, 128, lambda: _near_tie(N17, 128, 12803)),
    "hostile64": (262_144, 64, lambda: _hostile(262_144, 64, 6402, HOSTILE_NEEDLES)),
    "b32": (N17, 32, lambda: _featured(N17, 32, 3202, zero=False)),
    "b64": (N17, 64, lambda: _featured(N17, 64, 6403, zero=False)),
    "b64z": (N17, 64, lambda: _featured(N17, 64, 6403)),
    "b100": (N17, 100, lambda: _featured(N17, 100, 10003, zero=False)),
    "b113": (N17, 113, lambda: _featured(N17, 113, 11301, zero=False)),
    "b128": (N17, 128, lambda: _featured(N17, 128, 12804, zero=False)),
    "sub16": (N17, 64, lambda: _fp16_subnormal(N17, 64, 6404)),
    "n30": (N17, 30, lambda: _featured(N17, 30, 3001)),
    "n96": (N17, 96, lambda: _featured(N17, 96, 9601)),
    "px1024": (N17, 1024, lambda: _pixels(N17, 1024, 10241)),
    "p64": (N17 - 1, 64, lambda: _featured(N17 - 1, 64, 6405)),
    "p32": (N17 - 1, 32, lambda: _featured(N17 - 1, 32, 3203)),
    # the range cases: x * x an fp32 subnormal (2^-66: IEEE denormals, csrc/Makefile sets no flush flag), and large but finite (2^60)
    "n32lo": (N17, 32, lambda: table("n32") * np.float32(2.0 ** -66)),
    "n32hi": (N17, 32, lambda: table("n32") * np.float32(2.0 ** 60)),
    "n100lo": (N17, 100, lambda: table("n100") * np.float32(2.0 ** -66)),
    "n100hi": (N17, 100, lambda: table("n100") * np.float32(2.0 ** 60)),
    "p64lo": (N17 - 1, 64, lambda: table("p64") * np.float32(2.0 ** -66)),
    "p64hi": (N17 - 1, 64, lambda: table("p64") * np.float32(2.0 ** 60)),
}


def needles_for(Q, N):
    """Q needle rows: the anchors (row 0, row N - 1, row 1000 twice in one call), then rows spread over the table."""
    if Q == 1:
        return np.array([N - 1], dtype=np.int64)
    if Q == 2:
        return np.array([0, 0], dtype=np.int64)
    head = [0, 1000, N - 1, 1000]
    spread = [(i * 7919 + 11) % N for i in range(max(0, Q - len(head)))]
    return np.array((head + spread)[:Q], dtype=np.int64)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    table: str
    Q: int
    k: int
    accf: bool
    path: str              # what the case is about; the coverage test checks it against search_path()
    rerun: object = 0      # reruns the call must count: 0 or 1; None = reported, not asserted
    needles: tuple = None  # default: needles_for(Q, N)

    @property
    def N(self): return TABLES[self.table][0]

    @property
    def d(self): return TABLES[self.table][1]

    def rows(self):
        return np.array(self.needles, dtype=np.int64) if self.needles is not None else needles_for(self.Q, self.N)


CASES = [
    # small path: every D4 with accf both ways, NQ 2 / 5 / 8, k 1 / 50 / 128, N = 2^17 and ragged
    Case("small_d32_q1_k1", "n32", 1, 1, False, "small"),
    Case("small_d32_q6_k128_accf", "n32", 6, 128, True, "small"),
    Case("small_d64_q3_k50", "n64", 3, 50, False, "small"),
    Case("small_d64_q2_k128_accf", "n64", 2, 128, True, "small"),
    Case("small_d100_q3_k50_accf_ragged", "n100r", 3, 50, True, "small"),
    Case("small_d100_q8_k1", "n100", 8, 1, False, "small"),
    Case("small_d128_q8_k128_ragged", "n128r", 8, 128, False, "small"),
    Case("small_d128_q1_k50_accf", "n128", 1, 50, True, "small"),
    Case("small_near_tie", "near128", 2, 100, False, "small", needles=(1000, N17 - 1)),
    Case("small_near_tie_accf", "near128", 2, 100, True, "small", needles=(1000, N17 - 1)),
    # 262 144 rows: ~2048 persistent workgroups see 128 rows each, more than the 96 entries of a list (at 2^17 rows a list cannot overflow)
    Case("small_hostile_overflow", "hostile64", 5, 50, False, "small", rerun=1, needles=tuple(HOSTILE_NEEDLES)),
    # batched path: NK 2 / 4 / 7 / 8 (d = 113: scalar staging), Q = 32 and 2048 (qcap = 32, 80 904 bytes of LDS), k 1 / 128, N = 2^17
    Case("batched_d113_q32_k128", "b113", 32, 128, False, "batched"),
    Case("batched_d128_q2048_k128", "b128", 2048, 128, False, "batched", rerun=None),
    Case("batched_d128_q32_k1_accf", "b128", 32, 1, True, "batched"),
    Case("batched_d32_q48_k1", "b32", 48, 1, False, "batched"),
    Case("batched_d64_q40_k50_accf", "b64", 40, 50, True, "batched"),
    Case("batched_d100_q33_k128_accf", "b100", 33, 128, True, "batched"),
    Case("batched_zero_row", "b64z", 32, 50, False, "batched", rerun=1),
    Case("batched_fp16_subnormal_elements", "sub16", 32, 50, False, "batched", rerun=None),
    # filter path: Q past BQ_MAX, ragged needle groups (13 = 8 + 5, 9 = 8 + 1), DC 20 / 32, scalar staging, d = 1024, k 1 / 1024
    Case("filter_q2049_d128_k128", "b128", 2049, 128, False, "filter", rerun=None),
    Case("filter_d100_q13_k50_dc20", "n100", 13, 50, False, "filter"),
    Case("filter_d100_q9_k1024", "n100", 9, 1024, False, "filter", rerun=None),
    Case("filter_d96_q13_k1024_accf_dc32", "n96", 13, 1024, True, "filter", rerun=None),
    Case("filter_d30_q3_k1_accf", "n30", 3, 1, True, "filter"),
    Case("filter_d1024_q3_k100_pixels", "px1024", 3, 100, False, "filter"),
    # plain path: one row short of the filter
    Case("plain_n131071_q9_k1024", "p64", 9, 1024, False, "plain"),
    Case("plain_n131071_q2_k1_accf", "p32", 2, 1, True, "plain"),
    # input range, finite only: reruns allowed (every score equal to the next one at the approximate passes' resolution), exactness not
    Case("range_small_2m66", "n32lo", 5, 50, False, "small", rerun=None),
    Case("range_small_2p60", "n32hi", 5, 50, False, "small", rerun=None),
    Case("range_filter_2m66", "n100lo", 13, 50, False, "filter", rerun=None),
    Case("range_filter_2p60_accf", "n100hi", 13, 50, True, "filter", rerun=None),
    Case("range_plain_2m66", "p64lo", 9, 50, False, "plain"),
    Case("range_plain_2p60", "p64hi", 9, 50, False, "plain"),
]
BY_NAME = {c.name: c for c in CASES}

# the state sequence on one fresh context (test_small_path_state_across_calls); Q = 5 at d = 100 is the reference's five needles
SEQUENCE_EXTRA = [Case("small_d100_q5_k50", "n100", 5, 50, False, "small")]
BY_NAME.update({c.name: c for c in SEQUENCE_EXTRA})
SEQUENCE = ["small_d100_q5_k50", "small_hostile_overflow", "small_d64_q2_k128_accf", "small_d128_q8_k128_ragged", "plain_n131071_q2_k1_accf",
            "small_d100_q5_k50"]

# ---------------------------------------------------------------- references
_TABLE_CACHE, _REF_CACHE = {}, {}


def _kmax(table, accf):
    return max(c.k for c in list(CASES) + SEQUENCE_EXTRA if c.table == table and c.accf == accf)


def table(name):
    if name not in _TABLE_CACHE:
        if TABLES[name][1] * TABLES[name][0] > (1 << 26):     # (the 512 MB pixel table is not kept)
            return np.ascontiguousarray(TABLES[name][2](), dtype=np.float32)
        _TABLE_CACHE[name] = np.ascontiguousarray(TABLES[name][2](), dtype=np.float32)
    return _TABLE_CACHE[name]


def reference(oracle, case, emb):
    """(idx, scores) of oracle.cosine_topk for the case: per needle, computed once per (table, accf) at the largest k of that table."""
    cache = _REF_CACHE.setdefault((case.table, case.accf), {})
    rows = case.rows()
    todo = np.array(sorted(set(rows.tolist()) - set(cache)), dtype=np.int64)
    if todo.size:
        ri, rs = oracle_topk_parallel(oracle, emb, todo, _kmax(case.table, case.accf), case.accf)
        for j, r in enumerate(todo.tolist()):
            cache[r] = (ri[j], rs[j])
    return np.stack([cache[r][0][:case.k] for r in rows.tolist()]), np.stack([cache[r][1][:case.k] for r in rows.tolist()])


def assert_exact(case, idx, sc, ridx, rsc, what=""):
    assert idx.shape == ridx.shape == (case.Q, case.k), (case.name, idx.shape)
    bad = np.nonzero(~(idx == ridx).all(axis=1) | ~(sc == rsc).all(axis=1))[0]
    assert bad.size == 0, (f"{case.name}{what}: needles {bad[:8].tolist()} (rows {case.rows()[bad[:8]].tolist()}) differ from the oracle; first: "
                           f"got {idx[bad[0]][:8].tolist()} {sc[bad[0]][:8].tolist()}, want {ridx[bad[0]][:8].tolist()} {rsc[bad[0]][:8].tolist()}")
    assert np.all(sc[:, :-1] >= sc[:, 1:]), f"{case.name}: scores must be sorted descending"
    tie = sc[:, :-1] == sc[:, 1:]
    assert np.all(idx[:, :-1][tie] < idx[:, 1:][tie]), f"{case.name}: ties are ordered by ascending index"


def search(c, emb, case):
    return c.cosine_topk(emb, case.rows(), case.k, accumulate_in_float=case.accf)


def kernels_of_one_call(c, emb, case):
    """The call again under the per-kernel event timer: (idx, scores, kernel names it launched)."""
    c.set_timing(2)
    try:
        idx, sc = search(c, emb, case)
        names = {t["kernel"] for t in c.kernel_times()}
    finally:
        c.set_timing(0)
    return idx, sc, names - {"range_guard_fallback"}       # (a count of the trainer's range guard since gr_init, not a kernel)


# ---------------------------------------------------------------- tests
def test_case_table_reaches_every_leaf():
    """Every case is on the path search_path() gives it, and the table reaches every leaf of the dispatch tree: someone who adds a branch
    adds a case."""
    for c in CASES:
        assert search_path(c.N, c.d, c.Q, c.k) == c.path, (c.name, search_path(c.N, c.d, c.Q, c.k))
        assert c.rows().shape == (c.Q,) and c.rows().min() >= 0 and c.rows().max() < c.N, c.name
    on = {p: [c for c in CASES if c.path == p] for p in PATH_KERNELS}
    assert all(on.values()), "every path"
    assert {approx_d4(c.d) for c in on["small"]} == set(SMALL_D4), "every cos_approx_kernel D4"
    assert {approx_nq(c.Q) for c in on["small"]} == {2, 5, 8}, "every cos_approx_kernel NQ"
    assert {(approx_d4(c.d), c.accf) for c in on["small"]} == {(d4, a) for d4 in SMALL_D4 for a in (False, True)}, "every D4 with accf both ways"
    assert {mfma_nk(c.d) for c in on["batched"]} == {2, 4, 7, 8}, "every cos_mfma_kernel NK"
    assert {keys_dc(c.d) for c in on["filter"]} == {20, 32}, "both cos_keys_kernel DC on the filter path"
    assert {keys_dc(c.d) for c in on["filter"] if c.Q % QG} == {20, 32}, "a ragged needle group with both DC"
    for p, cs in on.items():
        assert {c.accf for c in cs} == {False, True}, f"accf both ways on the {p} path"
        assert 1 in {c.k for c in cs}, f"k = 1 on the {p} path"
        assert K_MAX[p] in {c.k for c in cs}, f"k = {K_MAX[p]} on the {p} path"
    qs = {c.Q for c in on["batched"]}
    assert BATCH_MIN_Q in qs and BQ_MAX in qs and BQ_MAX + 1 in {c.Q for c in on["filter"]}, "the batched path's needle limits"
    assert any(c.N == FILTER_MIN_ROWS - 1 for c in on["plain"]) and any(c.N == FILTER_MIN_ROWS for c in on["filter"]), "the filter's row limit"
    assert any(c.d > BD_MAX for c in on["filter"]) and any(c.d % 4 for c in on["filter"]) and any(c.d % 4 for c in on["batched"])
    assert {1, 2, 3, 6, 8} <= {c.Q for c in on["small"]} and {N17, 140_001} <= {c.N for c in on["small"]}
    assert any(c.rerun == 1 for c in on["small"]) and any(c.rerun == 1 for c in on["batched"]), "an overflow rerun from both list paths"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_search_path_bit_exact(ctx, oracle, case):
    """The case's result equals the oracle's bit for bit and is ordered (score descending, ties by ascending row); its reruns are as expected;
    the same call under the per-kernel timer launches exactly the kernels of the path search_path() predicts (plus the plain path's when it
    reruns) and returns the same bits."""
    emb = table(case.table)
    ridx, rsc = reference(oracle, case, emb)
    if case.name.startswith("small_near_tie"):
        cl = set(NEAR_CLUSTER.tolist()) | {1000, _dups(N17)[1000]}
        assert set(ridx[0].tolist()) <= cl and len(cl - set(ridx[0].tolist())) > 50 and float(rsc[0][0] - rsc[0][-1]) < 1e-6, \
            "the case: the needle's top 100 is part of the 202-row near-tie cluster, and the cluster straddles the cut"
    r0 = ctx.search_reruns()
    idx, sc = search(ctx, emb, case)
    reruns = ctx.search_reruns() - r0
    print(f"{case.name}: path {case.path}, reruns {reruns}")
    assert_exact(case, idx, sc, ridx, rsc)
    if case.rerun is not None:
        assert reruns == case.rerun, f"{case.name}: {reruns} reruns, expected {case.rerun}"
    r1 = ctx.search_reruns()
    tidx, tsc, names = kernels_of_one_call(ctx, emb, case)
    assert ctx.search_reruns() - r1 == reruns, f"{case.name}: the timed call reran {ctx.search_reruns() - r1} times, the untimed one {reruns}"
    want = PATH_KERNELS[case.path] | (PATH_KERNELS["plain"] if reruns else set())
    assert names == want, (f"{case.name}: the library launched {sorted(names)}; search_path() (the mirror of launch_cosine_topk's predicates in "
                           f"this file) predicts {sorted(want)} - update the mirror if search.hip's dispatch changed")
    assert np.array_equal(tidx, idx) and np.array_equal(tsc, sc), f"{case.name}: the timed call differs from the untimed one"


def test_small_path_state_across_calls(oracle):
    """The small path keeps state in the context between calls: the sample launch's arrival counter and histogram (left zero by every
    search), the pinned completion words and the call's sequence number.  On one fresh context: small Q = 5 -> the hostile table (lists
    overflow, rerun) -> small Q = 2 at d = 64 -> small Q = 8 at d = 128 -> a plain search -> small Q = 5 again.  Every call bit-exact, exactly
    one rerun, and the last call equal to the first."""
    import ganrev._lib as L
    c = L.Context(0)
    try:
        first = None
        r0 = c.search_reruns()
        for i, name in enumerate(SEQUENCE):
            case = BY_NAME[name]
            emb = table(case.table)
            ridx, rsc = reference(oracle, case, emb)
            idx, sc = search(c, emb, case)
            assert_exact(case, idx, sc, ridx, rsc, f" (call {i} of the sequence)")
            if first is None:
                first = (idx, sc)
        assert np.array_equal(idx, first[0]) and np.array_equal(sc, first[1])
        assert c.search_reruns() - r0 == 1, "only the hostile table reruns"
    finally:
        c.close()
