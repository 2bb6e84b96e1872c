"""The reference for a cosine top-k search whose needles are NOT rows of the table: append-and-filter on the unchanged oracle.

oracle.cosine_topk takes needle ROWS.  For outside vectors: append them to the table, search rows N .. N + Q - 1 of the appended table with
k + Q, drop every index >= N (the appended needles: there are Q of them, so at least k table rows remain among the first k + Q) and keep the
first k.  A (needle, row) score depends on those two vectors only and the order (score descending, index ascending) is total, so what is
left is exactly the top k of the table proper - it is also what parallel.sharded_cosine_topk does on every shard."""
import numpy as np

from helpers import oracle_topk_parallel


def append_and_filter(oracle, emb, needles, k, accumulate_in_float=False):
    """(idx int64 [Q, min(k, N)], scores float32) of the needle VECTORS `needles` [Q, d] over the rows of emb [N, d]"""
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    needles = np.ascontiguousarray(needles, dtype=np.float32).reshape(-1, emb.shape[1])
    N, Q = emb.shape[0], needles.shape[0]
    k = min(int(k), N)
    aug = np.concatenate([emb, needles])
    idx, sc = oracle_topk_parallel(oracle, aug, np.arange(N, N + Q, dtype=np.int64), k + Q, accumulate_in_float)
    out_i = np.empty((Q, k), np.int64); out_s = np.empty((Q, k), np.float32)
    for q in range(Q):
        keep = idx[q] < N
        assert int(keep.sum()) >= k
        out_i[q] = idx[q][keep][:k]; out_s[q] = sc[q][keep][:k]
    return out_i, out_s


def cosine_float64(emb, needles):
    """the scores [Q, N] restated in float64 numpy (no fp32 step): what the oracle's scores are within a few fp32 roundings of"""
    a = np.asarray(emb, np.float64); b = np.asarray(needles, np.float64)
    w = (1.0 / ((b * b).sum(1) + 1e-12))[:, None] * (1.0 / ((a * a).sum(1) + 1e-12))[None, :]
    return (b @ a.T) * np.sqrt(w)
