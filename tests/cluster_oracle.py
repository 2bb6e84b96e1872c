"""numpy restatement of gr_cluster_members_dev (include/ganrev.h states it; apply_r.lua:218-227): per cluster the member rows ordered by a
stable argsort of -similarity - similarity descending, ties by ascending row, NaN after every number - and the first m of them."""
import numpy as np


def cluster_members(labels, sims, k, m):
    """-> (rows int64 [k, m] with -1 fill, sims float32 [k, m] with 0 fill, kept int32 [k], sizes int32 [k])"""
    labels, sims = np.asarray(labels), np.asarray(sims, np.float32)
    rows_out = np.full((k, m), -1, np.int64)
    sims_out = np.zeros((k, m), np.float32)
    kept, sizes = np.zeros(k, np.int32), np.zeros(k, np.int32)
    for j in range(k):
        rows = np.nonzero(labels == j)[0]
        keep = rows[np.argsort(-sims[rows], kind="stable")][:m]
        sizes[j], kept[j] = len(rows), len(keep)
        rows_out[j, :len(keep)] = keep
        sims_out[j, :len(keep)] = sims[keep]
    return rows_out, sims_out, kept, sizes


def member_case(n, k, m, seed, nan=False):
    """labels / similarities for a selection test: cluster k-1 is empty (when k > 1), cluster 0 holds more than m rows (when n allows),
    and the similarities come from a handful of values, so that groups of exactly equal ones (with both zeros among them) cross the m
    cut-off and the tie rule decides who is kept."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, max(k - 1, 1), n).astype(np.int32)
    labels[rng.permutation(n)[: min(n, m + 9)]] = 0
    values = np.array([0.75, 0.5, 0.25, 0.0, -0.0, -0.5, 0.5000001, 1e-30], np.float32)
    sims = values[rng.integers(0, len(values), n)]
    if nan:
        sims[rng.permutation(n)[: max(2, n // 50)]] = np.nan
    return labels, sims
