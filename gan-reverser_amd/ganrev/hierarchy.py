"""Clustering without an eps: the exact minimum spanning tree of the recovered noise on the device, and the hierarchy read off it (no counterpart
in the reference, whose README ends its clustering section with "Maybe other clustering methods would produce better results": k-means, the
mixture and DBSCAN all ask for the parameter that decides the result - a cluster count, or a radius - and on a table whose groups differ in density
no single eps is right.  One spanning tree under the mutual-reachability distance is the whole single-linkage dendrogram: cut at any height it
gives DBSCAN*'s labels for every eps at once, and through the condensed tree it gives HDBSCAN's labels with no eps at all).

  mst         the exact minimum spanning tree of a table under max(dist, core_i, core_j) (gr_mst_dev; the core distances from ganrev.knn's
              graph, read where it lies) -> SpanningTree
  hdbscan     HDBSCAN's labels and membership probabilities of such a tree for one minClusterSize (gr_hdbscan_host) -> Clustering
  cluster     the two chained
  linkage     the tree as SciPy's [n - 1 x 4] linkage matrix, for scipy.cluster.hierarchy.dendrogram and fcluster
  cut         DBSCAN*'s labels at eps = height: the components of the edges with w <= height; rows with core > height are noise

The arithmetic, the edge order and scikit-learn's selection rules are stated in include/ganrev.h.  The tree is the n^2 d part - every pair is
visited once per Boruvka round, at most ceil(log2 n) rounds, at most 262144 rows - and is built where the table lies; mst waits on the stream once
per round.  Everything read off the tree's n - 1 edges is host work."""
import numpy as np

from . import _lib as L
from .nn_utils import DeviceScope, DeviceTensor, deviceTable

MAX_ROWS, MAX_COLUMNS = L.Context.MST_MAX_N, L.Context.MST_MAX_D
METRICS = tuple(sorted(L.Context.MST_METRICS))
MAX_MINSAMPLES = L.Context.KNN_MAX_K + 1        # core = column minSamples - 2 of a graph of k = minSamples - 1 <= 128 neighbours


class SpanningTree:
    """u, v [n - 1] int32, u < v, and w [n - 1] float64: the edges of the unique minimum spanning tree under the order (w, u, v), ascending by it;
    core [n] float64: every row's distance to its (minSamples - 1)-th nearest other row, or None for minSamples = 1 (plain single linkage);
    rounds: the Boruvka rounds taken; minSamples, metric as given"""

    def __init__(self, u, v, w, core=None, rounds=None, minSamples=1, metric=None):
        self.u, self.v, self.w, self.core = u, v, w, core
        self.rounds, self.minSamples, self.metric = rounds, int(minSamples), metric
        self.n = len(u) + 1


class Clustering:
    """labels [n] int32: the cluster of every row, 0 .. clusters - 1 in ascending order of the clusters' smallest member rows, -1 for noise; prob
    [n] float64: the membership strength, 0 for noise; clusters; sizes [clusters]: np.bincount of the labels; noise: the number of -1 rows"""

    def __init__(self, labels, prob, clusters, minClusterSize=None, minSamples=None, metric=None):
        self.labels, self.prob, self.clusters = labels, prob, int(clusters)
        self.minClusterSize, self.minSamples, self.metric = minClusterSize, minSamples, metric
        self.n = len(labels)
        self.sizes = np.bincount(labels[labels >= 0], minlength=self.clusters)
        self.noise = int((labels < 0).sum())
        self.tree = None


def checkShape(n, d, minSamples=1, metric="cosine"):
    if metric not in L.Context.MST_METRICS:
        raise L.GanrevError(f"hierarchy: metric {metric!r}: one of {sorted(L.Context.MST_METRICS)}")
    if not 2 <= int(n) <= MAX_ROWS:
        raise L.GanrevError(f"hierarchy: n {n}: 2 to {MAX_ROWS} rows (every pair of rows is visited)")
    if not 1 <= int(d) <= MAX_COLUMNS:
        raise L.GanrevError(f"hierarchy: d {d}: 1 to {MAX_COLUMNS} columns")
    if not 1 <= int(minSamples) <= min(int(n), MAX_MINSAMPLES):
        raise L.GanrevError(f"hierarchy: minSamples {minSamples}: 1 to min(n, {MAX_MINSAMPLES}) = {min(int(n), MAX_MINSAMPLES)} "
                            "(the row itself and its minSamples - 1 nearest rows)")


def checkMinClusterSize(n, minClusterSize):
    if not 2 <= int(minClusterSize) <= int(n):
        raise L.GanrevError(f"hierarchy: minClusterSize {minClusterSize}: 2 to n = {n} rows")


def _asTable(ctx, table, rows, who):
    if isinstance(table, tuple):
        ptr, N, d = table
        table = DeviceTensor(ctx, (N, d), ptr)                                # a view: the caller keeps the memory
    elif not isinstance(table, DeviceTensor):
        table = np.asarray(table, np.float32)
    if rows is not None and not 0 < int(rows) <= table.shape[0]:
        raise L.GanrevError(f"{who}: rows {rows}: the first rows of a table of {table.shape[0]}")
    return table


def mst(ctx, table, minSamples=1, metric="cosine", rows=None):
    """The minimum spanning tree of `table`: a DeviceTensor [N x d], a (pointer, N, d) triple, or a host array [N x d], uploaded to a temporary
    buffer first as deviceTable does.  rows=M: the tree of the first M rows alone.  minSamples is DBSCAN's minPts, the row itself included: 1 is
    plain single linkage; 2 to 129 builds ganrev.knn's graph with k = minSamples - 1, kept on the device, whose last column - the core distances -
    is read in place.  Waits on the stream once per Boruvka round.  -> SpanningTree"""
    from . import knn as KNN
    table = _asTable(ctx, table, rows, "hierarchy.mst")
    with deviceTable(ctx, table, rows=None if rows is None else int(rows)) as (ptr, n, d), DeviceScope(ctx) as own:
        checkShape(n, d, minSamples, metric)
        k = int(minSamples) - 1
        core_dev, core = None, None
        if k:
            g = own.adopt(KNN.graph(ctx, (ptr, n, d), k, metric, keep=True))
            core_dev = g.dist_dev + 8 * (k - 1)                               # column k - 1 of dist [n x k], stride k
        u, v, w = own.malloc(4 * (n - 1)), own.malloc(4 * (n - 1)), own.malloc(8 * (n - 1))
        rounds = ctx.mst_dev(ptr, n, d, metric, core_dev, max(k, 1), u, v, w)
        if k:
            core = np.ascontiguousarray(ctx.download(g.dist_dev, (n, k), np.float64)[:, k - 1])
        return SpanningTree(ctx.download(u, (n - 1,), np.int32), ctx.download(v, (n - 1,), np.int32), ctx.download(w, (n - 1,), np.float64),
                            core, rounds, minSamples, metric)


def hdbscan(tree, minClusterSize):
    """-> Clustering of a SpanningTree for one minClusterSize in [2, n]: scikit-learn's HDBSCAN at its defaults (excess of mass, the root never
    selected).  One tree serves any minClusterSize.  Host work; needs no GPU"""
    checkMinClusterSize(tree.n, minClusterSize)
    labels, prob, clusters = L.hdbscan_host(tree.u, tree.v, tree.w, tree.n, int(minClusterSize))
    return Clustering(labels, prob, clusters, int(minClusterSize), tree.minSamples, tree.metric)


def cluster(ctx, table, minSamples, minClusterSize, metric="cosine", rows=None):
    """mst, then hdbscan -> Clustering, whose .tree is the SpanningTree"""
    table = _asTable(ctx, table, rows, "hierarchy.cluster")
    n = table.shape[0] if rows is None else int(rows)
    checkShape(n, table.shape[1] if len(table.shape) > 1 else 0, minSamples, metric)
    checkMinClusterSize(n, minClusterSize)
    tree = mst(ctx, table, minSamples, metric, rows)
    c = hdbscan(tree, minClusterSize)
    c.tree = tree
    return c


def _find(up, a):
    r = a
    while up[r] != r:
        r = up[r]
    while up[a] != r:
        up[a], a = r, up[a]
    return r


def linkage(tree):
    """-> [n - 1 x 4] float64 in SciPy's format: row k joins the clusters (lower number first) that the tree's k-th edge connects, at height w[k],
    into cluster n + k of the given row count"""
    n = tree.n
    up, node, count = list(range(n)), list(range(n)), [1] * n
    Z = np.zeros((n - 1, 4))
    for k, (a, b, w) in enumerate(zip(tree.u.tolist(), tree.v.tolist(), tree.w.tolist())):
        ra, rb = _find(up, a), _find(up, b)
        if ra == rb:
            raise L.GanrevError(f"hierarchy.linkage: edge {k} ({a}, {b}) closes a cycle: not a spanning tree")
        Z[k] = min(node[ra], node[rb]), max(node[ra], node[rb]), w, count[ra] + count[rb]
        up[rb], node[ra], count[ra] = ra, n + k, count[ra] + count[rb]
    return Z


def cut(tree, height):
    """DBSCAN* at eps = height -> labels [n] int32: the connected components of the tree's edges with w <= height, numbered by their smallest
    member row; a row whose core distance is above height is noise, -1 (with minSamples = 1 every row is core, and a row alone is its own cluster)"""
    if not (np.isfinite(height) and float(height) >= 0):
        raise L.GanrevError(f"hierarchy.cut: height {height}: a finite distance, not below 0")
    n = tree.n
    up = list(range(n))
    below = tree.w <= float(height)
    for a, b in zip(tree.u[below].tolist(), tree.v[below].tolist()):
        ra, rb = _find(up, a), _find(up, b)
        up[max(ra, rb)] = min(ra, rb)                                         # every component under its smallest row
    core = np.ones(n, bool) if tree.core is None else tree.core <= float(height)
    labels, number = np.full(n, -1, np.int32), {}
    for i in np.nonzero(core)[0].tolist():
        labels[i] = number.setdefault(_find(up, i), len(number))
    return labels
