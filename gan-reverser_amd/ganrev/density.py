"""Density-based clustering of the recovered noise, on the device: DBSCAN (no counterpart in the reference, whose README ends its clustering section
with "Maybe other clustering methods would produce better results": k-means and the mixture force a cluster count on the table, split elongated
groups and give every row a cluster; this one finds the count itself, follows groups of any shape and labels the rows that belong nowhere as
noise, -1 - the set-level counterpart of the local outlier factor).

  epsGraph            the eps-neighbourhood graph of a table as a bitmap that stays on the device (gr_eps_graph_dev) -> DeviceEpsGraph
  dbscan              DBSCAN's labels of such a graph for one minPts (gr_dbscan_dev) -> Clustering; one graph serves any minPts
  cluster             the two chained
  epsFromNeighbours   the k-distance rule for eps: a quantile of every row's distance to its (minPts - 1)-th nearest row (ganrev.knn)

The arithmetic and the labelling rule - scikit-learn's - are stated in include/ganrev.h; everything runs where the table lies.  All pairs are
visited: n^2 d work and n^2 / 8 bytes of bitmap, at most 262144 rows.  dbscan waits on the stream once per round of its component search.
"""
import numpy as np

from . import _lib as L
from .nn_utils import DeviceScope, DeviceTensor, deviceTable

MAX_ROWS, MAX_COLUMNS = L.Context.DBSCAN_MAX_N, L.Context.DBSCAN_MAX_D
METRICS = tuple(sorted(L.Context.DBSCAN_METRICS))
MAX_MINPTS_BY_NEIGHBOURS = L.Context.KNN_MAX_K + 1      # epsFromNeighbours reads column minPts - 2 of a graph of k = minPts - 1 <= 128 neighbours


class EpsGraph:
    """words [n x ceil(n / 64)] uint64: bit j % 64 of word j / 64 of row i is set iff dist(i, j) <= eps (the diagonal always); count [n] int32:
    the rows' popcounts, the row itself included; eps, metric as given"""

    def __init__(self, words, count, eps=None, metric=None):
        self.words, self.count, self.eps, self.metric = words, count, eps, metric
        self.n = len(count)

    def dense(self):
        """-> [n x n] bool"""
        bits = np.unpackbits(np.ascontiguousarray(self.words).view(np.uint8), axis=1, bitorder="little")
        return bits[:, :self.n].astype(bool)


class DeviceEpsGraph:
    """An EpsGraph where gr_eps_graph_dev left it: adj_dev [n x words] uint64, count_dev [n] int32.  numpy() copies it to the host; close() (or
    leaving a `with` block over it) frees it."""

    def __init__(self, ctx, n, eps=None, metric=None):
        self.ctx, self.n, self.eps, self.metric = ctx, int(n), eps, metric
        self.words = L.Context.eps_words(self.n)
        self.mem = DeviceScope(ctx)
        self.adj_dev, self.count_dev = self.mem.malloc(8 * self.n * self.words), self.mem.malloc(4 * self.n)

    def numpy(self):
        return EpsGraph(self.ctx.download(self.adj_dev, (self.n, self.words), np.uint64), self.ctx.download(self.count_dev, (self.n,), np.int32),
                        self.eps, self.metric)

    def close(self):
        self.mem.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Clustering:
    """labels [n] int32: the cluster of every row, 0 .. clusters - 1 in ascending order of the clusters' smallest core rows, -1 for noise; core
    [n] bool; count [n] int32: the rows' neighbourhood sizes, themselves included; clusters; sizes [clusters]: np.bincount of the labels"""

    def __init__(self, labels, core, count, clusters, minPts=None, eps=None, metric=None):
        self.labels, self.core, self.count, self.clusters = labels, core, count, int(clusters)
        self.minPts, self.eps, self.metric = minPts, eps, metric
        self.n = len(labels)
        self.sizes = np.bincount(labels[labels >= 0], minlength=self.clusters)
        self.noise = int((labels < 0).sum())
        self.border = int(((labels >= 0) & ~core).sum())


def checkShape(n, d, eps=0.0, minPts=1, metric="cosine"):
    if metric not in L.Context.DBSCAN_METRICS:
        raise L.GanrevError(f"density: metric {metric!r}: one of {sorted(L.Context.DBSCAN_METRICS)}")
    if not 2 <= int(n) <= MAX_ROWS:
        raise L.GanrevError(f"density: n {n}: 2 to {MAX_ROWS} rows (every pair of rows is visited)")
    if not 1 <= int(d) <= MAX_COLUMNS:
        raise L.GanrevError(f"density: d {d}: 1 to {MAX_COLUMNS} columns")
    if not (np.isfinite(eps) and float(eps) >= 0):
        raise L.GanrevError(f"density: eps {eps}: a finite distance, not below 0")
    if not 1 <= int(minPts) <= int(n):
        raise L.GanrevError(f"density: minPts {minPts}: 1 to n = {n} rows (a neighbourhood holds no more)")


def _asTable(ctx, table, rows, who):
    if isinstance(table, tuple):
        ptr, N, d = table
        table = DeviceTensor(ctx, (N, d), ptr)                                # a view: the caller keeps the memory
    elif not isinstance(table, DeviceTensor):
        table = np.asarray(table, np.float32)
    if rows is not None and not 0 < int(rows) <= table.shape[0]:
        raise L.GanrevError(f"{who}: rows {rows}: the first rows of a table of {table.shape[0]}")
    return table


def epsGraph(ctx, table, eps, metric="cosine", rows=None):
    """The eps-neighbourhood graph of `table`: a DeviceTensor [N x d], a (pointer, N, d) triple, or a host array [N x d], uploaded to a temporary
    buffer first as deviceTable does.  rows=M: the graph of the first M rows alone.  -> DeviceEpsGraph, which the caller closes"""
    table = _asTable(ctx, table, rows, "density.epsGraph")
    with deviceTable(ctx, table, rows=None if rows is None else int(rows)) as (ptr, n, d):
        checkShape(n, d, eps, 1, metric)
        g = DeviceEpsGraph(ctx, n, float(eps), metric)
        try:
            ctx.eps_graph_dev(ptr, n, d, eps, metric, g.adj_dev, g.count_dev)
            return g
        except Exception:
            g.close()
            raise


def dbscan(ctx, graph, minPts):
    """-> Clustering of a DeviceEpsGraph (or an EpsGraph, uploaded for the call) for one minPts.  Waits on the stream once per round of the
    component search."""
    if not 1 <= int(minPts) <= graph.n:
        raise L.GanrevError(f"density.dbscan: minPts {minPts}: 1 to n = {graph.n} rows (a neighbourhood holds no more)")
    n = graph.n
    with DeviceScope(ctx) as own:
        if isinstance(graph, DeviceEpsGraph):
            adj, count = graph.adj_dev, graph.count_dev
        else:
            adj, count = own.upload(np.ascontiguousarray(graph.words, np.uint64)), own.upload(np.ascontiguousarray(graph.count, np.int32))
        labels, core, clusters = own.malloc(4 * n), own.malloc(4 * n), own.malloc(4)
        ctx.dbscan_dev(adj, count, n, int(minPts), labels, core, clusters)
        return Clustering(ctx.download(labels, (n,), np.int32), ctx.download(core, (n,), np.int32).astype(bool), ctx.download(count, (n,), np.int32),
                          int(ctx.download(clusters, (1,), np.int32)[0]), int(minPts), graph.eps, graph.metric)


def cluster(ctx, table, eps, minPts, metric="cosine", rows=None):
    """epsGraph, then dbscan -> Clustering"""
    table = _asTable(ctx, table, rows, "density.cluster")
    n = table.shape[0] if rows is None else int(rows)
    checkShape(n, table.shape[1] if len(table.shape) > 1 else 0, eps, minPts, metric)
    with epsGraph(ctx, table, eps, metric, rows) as g:
        return dbscan(ctx, g, minPts)


def epsFromNeighbours(ctx, table, minPts, quantile=0.75, metric="cosine", rows=None):
    """The k-distance rule: every row's distance to its (minPts - 1)-th nearest other row (column minPts - 2 of ganrev.knn's graph of
    k = minPts - 1 neighbours), and its `quantile`-quantile as eps -> (eps, kdist [n] float64).  The pair distances are the same bits in both
    calls, so exactly the rows with kdist <= eps are core at that eps and minPts: about the share `quantile` of them.  2 <= minPts <= 129."""
    from . import knn as KNN
    if not 2 <= int(minPts) <= MAX_MINPTS_BY_NEIGHBOURS:
        raise L.GanrevError(f"density.epsFromNeighbours: minPts {minPts}: 2 to {MAX_MINPTS_BY_NEIGHBOURS} (the distance to the (minPts - 1)-th neighbour)")
    if not 0 <= float(quantile) <= 1:
        raise L.GanrevError(f"density.epsFromNeighbours: quantile {quantile}: 0 to 1")
    with KNN.graph(ctx, table, int(minPts) - 1, metric, rows=rows, keep=True) as g:
        kdist = np.ascontiguousarray(g.numpy().dist[:, -1])
    return float(np.quantile(kdist, float(quantile))), kdist
