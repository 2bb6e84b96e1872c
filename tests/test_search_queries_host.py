"""not-gpu: the host-side parts of search by example - the append-and-filter reference the GPU tests compare with, the sharded search
without the concatenation, and apply_r's two options that read --dataset."""
import numpy as np
import pytest

from helpers import tied_corpus
from search_queries_oracle import append_and_filter, cosine_float64


def _rng(seed):
    return np.random.default_rng(seed)


# ---------------------------------------------------------------- the reference itself
def test_append_and_filter_equals_the_row_search_for_a_copied_row(oracle):
    emb = _rng(1).standard_normal((3000, 24), dtype=np.float32)
    emb[2100] = emb[17]                                     # a duplicate: ties on index
    for accf in (False, True):
        for r in (0, 17, 2100, 2999):
            ri, rs = oracle.cosine_topk(emb, [r], 40, accumulate_in_float=accf)
            gi, gs = append_and_filter(oracle, emb, emb[r:r + 1].copy(), 40, accf)
            assert np.array_equal(gi, ri) and np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), (r, accf)


def test_append_and_filter_against_float64_numpy_with_ties(oracle):
    """200 x 7, duplicate rows and a zero row: the order is the float64 order wherever float64 separates two scores by more than fp32
    rounding, equal vectors come in index order, nothing better is left out, and a zero needle returns rows 0 .. k-1 with score 0."""
    rng = _rng(2)
    emb = rng.integers(-3, 4, size=(200, 7)).astype(np.float32)
    emb[emb.any(axis=1) == 0] = 1.0
    emb[50] = emb[7]; emb[120] = emb[7]; emb[199] = emb[0]  # exact ties
    emb[33] = 0.0                                           # a zero row: score 0 against everything
    needles = np.stack([emb[7] * np.float32(0.5), rng.standard_normal(7).astype(np.float32), emb[0] + np.float32(0.25), np.zeros(7, np.float32)])
    k, tol = 60, 1e-6
    idx, sc = append_and_filter(oracle, emb, needles, k)
    s64 = cosine_float64(emb, needles)
    for q in range(len(needles)):
        got = s64[q][idx[q]]
        assert len(set(idx[q].tolist())) == k
        assert np.all(np.abs(sc[q] - got) <= tol), q
        assert np.all(got[:-1] >= got[1:] - tol), q                                   # float64 order up to fp32 rounding
        rest = np.setdiff1d(np.arange(200), idx[q])
        assert s64[q][rest].max() <= got[-1] + tol, q                                  # nothing better left out
        same = (sc[q][:-1] == sc[q][1:])
        assert np.all(idx[q][:-1][same] < idx[q][1:][same]), q                         # ties by ascending index
        for a, b in ((7, 50), (50, 120), (0, 199)):                                    # bit-equal rows: equal scores, index order
            pa, pb = np.nonzero(idx[q] == a)[0], np.nonzero(idx[q] == b)[0]
            if len(pb):
                assert len(pa) and pa[0] < pb[0] and sc[q][pa[0]] == sc[q][pb[0]], (q, a, b)
    assert np.array_equal(idx[3], np.arange(k)) and not sc[3].any()
    assert idx[0][:3].tolist() == [7, 50, 120]


# ---------------------------------------------------------------- the sharded search without the concatenation
def _oracle_queries(oracle):
    return lambda emb, needles, k: append_and_filter(oracle, emb, needles, k)


def _sharded_queries_in_process(local, emb, bounds, needles, k):
    """sharded_cosine_topk_queries for every shard, one after the other: each rank's candidates are caught at its all-gather and merged as
    the ranks would (helpers.sharded_search_in_process does the same for the row-index version)"""
    from ganrev.parallel import merge_candidates, sharded_cosine_topk_queries

    class Comm:
        def __init__(self): self.got = []
        def allgather(self, arr):
            self.got.append(arr); return [arr]
    ci, cs = [], []
    for lo, hi in bounds:
        c = Comm()
        sharded_cosine_topk_queries(local, emb[lo:hi], lo, needles, k, c)
        ci.append(c.got[0]); cs.append(c.got[1])
    return merge_candidates(ci, cs, k)


def _bounds(N, parts):
    cuts = [0] + sorted({(N * (i + 1)) // parts + (3 * i) % 5 for i in range(parts - 1)}) + [N]
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("parts", [1, 3, 8])
def test_sharded_queries_equal_the_sharded_row_search(oracle, parts):
    """Needles gathered by gather_needles (here: the rows themselves): the same lists, bit for bit, as sharded_cosine_topk, with tie
    groups across shard boundaries (helpers.tied_corpus wants four shards: the 8-shard run) and plain tables otherwise"""
    from helpers import sharded_search_in_process
    N, d, k = 1600, 12, 30
    bounds = _bounds(N, parts)
    needle = bounds[0][0] + 3
    if parts >= 4:
        emb, _ = tied_corpus(N, d, 5, needle, bounds)
    else:
        emb = _rng(6).standard_normal((N, d), dtype=np.float32)
        emb[N - 5] = emb[needle]; emb[N // 2] = emb[needle]
    rows = [needle, N - 1, 700, needle]
    want = sharded_search_in_process(oracle.cosine_topk, emb, bounds, rows, k)
    got = _sharded_queries_in_process(_oracle_queries(oracle), emb, bounds, emb[rows].copy(), k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    whole = oracle.cosine_topk(emb, rows, k)
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


def test_sharded_queries_with_fewer_than_k_rows_in_a_shard(oracle):
    from helpers import sharded_search_in_process
    emb = _rng(7).standard_normal((64, 9), dtype=np.float32)
    bounds = [(0, 5), (5, 6), (6, 64)]                     # shards of 5 and 1 rows, k = 20
    rows = [2, 5, 63]
    want = sharded_search_in_process(oracle.cosine_topk, emb, bounds, rows, 20)
    got = _sharded_queries_in_process(_oracle_queries(oracle), emb, bounds, emb[rows].copy(), 20)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    # one communicator for the whole corpus (world 1), and fewer than k rows in all: the lists end in -1 / -inf like the row-index version's
    from ganrev.parallel import LocalCommunicator, sharded_cosine_topk, sharded_cosine_topk_queries
    a = sharded_cosine_topk(oracle.cosine_topk, emb[:7], 0, [2, 5], 20, LocalCommunicator())
    b = sharded_cosine_topk_queries(_oracle_queries(oracle), emb[:7], 0, emb[[2, 5]].copy(), 20, LocalCommunicator())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (b[0][:, 7:] == -1).all()


# ---------------------------------------------------------------- apply_r's options
def test_apply_r_parse_refuses_the_options_without_a_dataset_or_with_host(tmp_path):
    from ganrev import apply_r
    for opts in (["--needles", "3"], ["--real"]):
        with pytest.raises(SystemExit):
            apply_r.parse(opts)
        with pytest.raises(SystemExit):
            apply_r.parse(opts + ["--dataset", str(tmp_path), "--host"])
        assert apply_r.parse(opts + ["--dataset", str(tmp_path)]).dataset == str(tmp_path)
    with pytest.raises(SystemExit):
        apply_r.parse(["--needles", "-1", "--dataset", str(tmp_path)])


def test_apply_r_parse_without_the_options_is_what_it_was():
    from ganrev import apply_r
    got = vars(apply_r.parse([]))
    assert got.pop("needles") == 0 and got.pop("real") is False
    assert got == {"batchSize": 32, "seed": 1, "gpu": 0, "G": "logs/adversarial.net", "R": "logs/r_3x32x32_nd32_normal.net",
                   "R_fixer": "logs/r_3x32x32_nd32_normal_fixer.net", "writeTo": "r_results", "nbImages": 10000, "synthetic": "", "host": False,
                   "dataset": "NONE", "fileExtension": "jpg", "cacheDataset": None, "conv_mode": "f16x3", "quiet": False, "resident": False,
                   "render": False, "refine": 0, "refine_lr": 0.01}
