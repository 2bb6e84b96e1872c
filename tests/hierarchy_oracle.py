"""float64 numpy reference of gr_mst_dev and gr_hdbscan_host (include/ganrev.h) in their direct form: every pair's distance by the textbook
formulas (density_oracle.distances: no chain order, no tiles), the core distances from a full sort of every row, the minimum spanning tree by
Kruskal over ALL pairs sorted by (w, lo, hi) - no rounds, no components' minima - and HDBSCAN as it is usually told: the dendrogram as nested
merges, a recursive walk that condenses it, every cluster's (lambda, size) records summed by math.fsum, and the excess-of-mass choice by a
recursion from the root.  Plain Python and numpy: no sklearn, no scipy."""
import math
import sys

import numpy as np

import density_oracle as do
from silhouette_oracle import METRICS  # noqa: F401  (for the tests)


def distances(x, metric):
    """[n x n], symmetric bit for bit: the upper triangle of density_oracle.distances, mirrored (a matrix-vector product need not give dist_ij and
    dist_ji the same last bit; the library's chain does, and so must the reference, or a tie of the one is a near-tie of the other)"""
    dist = do.distances(x, metric)
    upper = np.triu(dist, 1)
    return upper + upper.T


def core_distances(dist, min_samples):
    """[n]: every row's distance to its (min_samples - 1)-th nearest other row, from a full sort; None for min_samples 1"""
    if min_samples < 2:
        return None
    off = np.array(dist, np.float64)
    np.fill_diagonal(off, np.inf)
    return np.sort(off, axis=1)[:, min_samples - 2].copy()


def weights(dist, core):
    """[n x n]: max(dist_ij, core_i, core_j); dist itself without core distances"""
    if core is None:
        return np.array(dist, np.float64)
    return np.maximum(np.maximum(dist, core[:, None]), core[None, :])


def kruskal(w):
    """-> (u, v, weight) [n - 1]: the minimum spanning tree of the complete graph under the order (w, lo, hi), its edges ascending by it"""
    n = len(w)
    lo, hi = np.triu_indices(n, 1)
    order = np.lexsort((hi, lo, w[lo, hi]))
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    u, v, weight = [], [], []
    for e in order.tolist():
        a, b = find(int(lo[e])), find(int(hi[e]))
        if a != b:
            root[a] = b
            u.append(int(lo[e])); v.append(int(hi[e])); weight.append(float(w[lo[e], hi[e]]))
            if len(u) == n - 1:
                break
    return np.array(u, np.int64), np.array(v, np.int64), np.array(weight, np.float64)


def tree(x, min_samples, metric, dist=None):
    """-> dict(u, v, w, core, dist)"""
    dist = distances(x, metric) if dist is None else dist
    core = core_distances(dist, min_samples)
    u, v, w = kruskal(weights(dist, core))
    return dict(u=u, v=v, w=w, core=core, dist=dist)


class Cluster:
    def __init__(self, birth, parent):
        self.birth, self.parent, self.records, self.rows, self.children = birth, parent, [], [], []

    def stability(self):
        return math.fsum((lam - self.birth) * size if lam != self.birth else 0.0 for lam, size in self.records)

    def lambda_max(self):
        return max(lam for lam, _ in self.records)


def hdbscan(u, v, w, n, min_cluster_size):
    """-> dict(labels [n] int64, prob [n], clusters; compared: per excess-of-mass comparison (the children's total, the cluster's own stability,
    the Cluster); row_lambda, top_lambda [n]: the lambda a row fell out at and the largest lambda of its selected cluster, 0 for noise;
    all_clusters: every Cluster of the condensed tree, the root first)"""
    # the dendrogram, as nested tuples (left, right, height, rows) over leaves that are ints
    top = {i: i for i in range(n)}
    rows_of = {i: [i] for i in range(n)}
    root = list(range(n))

    def find(a):
        while root[a] != a:
            a = root[a]
        return a

    for a, b, h in zip(u.tolist(), v.tolist(), w.tolist()):
        ra, rb = find(a), find(b)
        assert ra != rb
        node = (top[ra], top[rb], h, rows_of[ra] + rows_of[rb])
        root[rb] = ra
        top[ra], rows_of[ra] = node, node[3]
    dendrogram = top[find(0)]
    size = lambda node: 1 if isinstance(node, int) else len(node[3])
    members = lambda node: [node] if isinstance(node, int) else node[3]

    clusters = [Cluster(0.0, None)]
    fell = {}                                                           # row -> (cluster, lambda)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * n + 100))

    def condense(node, c):
        left, right, h, _ = node
        lam = 1.0 / h if h > 0 else math.inf
        big = [size(s) >= min_cluster_size for s in (left, right)]
        if all(big):
            for side in (left, right):
                child = Cluster(lam, c)
                clusters.append(child); c.children.append(child); c.records.append((lam, size(side)))
                condense(side, child)
            return
        for side, keeps in zip((left, right), big):
            if keeps:
                condense(side, c)
            else:
                c.records.append((lam, size(side)))
                for r in members(side):
                    fell[r] = (c, lam)

    try:
        condense(dendrogram, clusters[0])
        compared = []

        def best(c):
            """the largest total stability of a choice of clusters inside c, c itself among the candidates -> (total, the chosen)"""
            own = c.stability()
            if not c.children:
                return own, [c]
            below = [best(k) for k in c.children]
            total = below[0][0] + below[1][0]
            compared.append((total, own, c))
            return (total, below[0][1] + below[1][1]) if total > own else (own, [c])

        chosen = []
        for k in clusters[0].children:                                  # the root is never a cluster
            chosen += best(k)[1]
    finally:
        sys.setrecursionlimit(limit)
    owner = {}
    for c in chosen:
        stack = [c]
        while stack:
            k = stack.pop()
            owner[id(k)] = c
            stack += k.children
    labels, prob, number = np.full(n, -1, np.int64), np.zeros(n), {}
    row_lambda, top_of_row = np.zeros(n), np.zeros(n)
    for r in range(n):
        c, lam = fell[r]
        c = owner.get(id(c))
        if c is None:
            continue
        labels[r] = number.setdefault(id(c), len(number))
        top_lambda = c.lambda_max()
        row_lambda[r], top_of_row[r] = lam, top_lambda
        with np.errstate(invalid="ignore"):
            q = np.float64(min(lam, top_lambda)) / np.float64(top_lambda)
        prob[r] = q if np.isfinite(q) else 1.0
    return dict(labels=labels, prob=prob, clusters=len(number), compared=compared, all_clusters=clusters, row_lambda=row_lambda, top_lambda=top_of_row)
