"""float64 numpy reference of gr_eps_graph_dev and gr_dbscan_dev (include/ganrev.h) in their direct form: every pair's distance by the textbook
formulas (silhouette_oracle.distances_from: no chain order, no tiles), the neighbourhoods by one comparison, and DBSCAN as it is usually written:
a breadth-first expansion from every unvisited core row in row order.  Plain Python and numpy: no sklearn, no scipy."""
from collections import deque

import numpy as np

from silhouette_oracle import METRICS, distances_from  # noqa: F401  (METRICS: for the tests)


def distances(x, metric):
    """[n x n]: the distance of every pair; the diagonal is 0"""
    assert metric in METRICS
    X = np.asarray(x, np.float64)
    norms = np.sqrt((X * X).sum(axis=1))
    return np.stack([distances_from(X, norms, i, metric) for i in range(len(X))])


def neighbourhoods(dist, eps):
    """-> (adj [n x n] bool: dist <= eps, and every row in its own; count [n]: the rows' neighbourhood sizes, themselves included)"""
    adj = np.asarray(dist) <= eps
    np.fill_diagonal(adj, True)
    return adj, adj.sum(axis=1)


def kdistances(dist, k):
    """[n]: every row's distance to its k-th nearest other row (k >= 1)"""
    off = np.array(dist, np.float64)
    np.fill_diagonal(off, np.inf)
    return np.partition(off, k - 1, axis=1)[:, k - 1]


def dbscan(adj, min_pts):
    """-> (labels [n] int64, -1 noise; core [n] bool; the number of clusters): every unvisited core row, in row order, opens a cluster and the
    cluster grows breadth-first through core rows; a row that is not core joins the first cluster that reaches it and carries it no further"""
    adj = np.asarray(adj, bool)
    n = len(adj)
    core = adj.sum(axis=1) >= min_pts
    labels = np.full(n, -1, np.int64)
    clusters = 0
    for seed in range(n):
        if not core[seed] or labels[seed] >= 0:
            continue
        labels[seed] = clusters
        queue = deque([seed])
        while queue:
            p = queue.popleft()
            for q in np.nonzero(adj[p])[0]:
                if labels[q] < 0:
                    labels[q] = clusters
                    if core[q]:
                        queue.append(int(q))
        clusters += 1
    return labels, core, clusters
