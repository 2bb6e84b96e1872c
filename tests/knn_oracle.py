"""float64 numpy reference of gr_knn_dev, gr_lof_dev and gr_knn_overlap_dev (include/ganrev.h) in their direct form: a row's distances to all rows
(silhouette_oracle.distances_from), sorted by numpy's lexsort by distance, then index; the local outlier factor by numpy's means; the overlap by
sets.  No tiles, no lists, no chain order."""
import numpy as np

from silhouette_oracle import METRICS, distances_from  # noqa: F401  (METRICS: for the tests)


def knn(x, k, metric):
    """-> dict(idx [n x k] int64, dist [n x k]: row i's k nearest rows j != i by (distance, j) ascending; ahead [n x min(k + 1, n - 1)]: the
    distances of the first k + 1 neighbours where the table has that many - what decides a row's list)"""
    assert metric in METRICS
    X = np.asarray(x, np.float64)
    n = len(X)
    assert 1 <= k <= n - 1
    norms = np.sqrt((X * X).sum(axis=1))
    m = min(k + 1, n - 1)
    idx, ahead = np.zeros((n, k), np.int64), np.zeros((n, m))
    for i in range(n):
        dist = distances_from(X, norms, i, metric)
        dist[i] = np.inf                                                # a row is not its own neighbour
        order = np.lexsort((np.arange(n), dist))[:m]
        idx[i], ahead[i] = order[:k], dist[order]
    return dict(idx=idx, dist=ahead[:, :k].copy(), ahead=ahead)


def lof(idx, dist):
    """-> (lof, lrd) [n] of a graph: kdist_j = dist[j][k - 1], reach(i, j) = max(kdist_j, dist[i][p]), lrd = 1 / (mean reach + 1e-10),
    lof = mean of the neighbours' lrd / lrd"""
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.float64)
    reach = np.maximum(dist[:, -1][idx], dist)
    lrd = 1.0 / (reach.mean(axis=1) + 1e-10)
    return lrd[idx].mean(axis=1) / lrd, lrd


def overlap(idx_a, idx_b):
    """-> (count [n]: the entries of a's row i that occur in b's row i, the mean of count / k)"""
    count = np.array([len(set(a.tolist()) & set(b.tolist())) for a, b in zip(np.asarray(idx_a), np.asarray(idx_b))], np.int64)
    return count, float((count / np.asarray(idx_a).shape[1]).mean())
