"""The exact k-nearest-neighbour graph of the recovered noise, on the device, and what is read off it (no counterpart in the reference, whose README
has an anomaly section: the local outlier factor is the non-parametric answer to it - a row's neighbour density against its neighbours', from
nothing but every row's k nearest rows - and the share of a row's neighbours that a map or a projection keeps is the number that says whether the
picture can be believed).

  graph        every row's k nearest other rows and their distances (gr_knn_dev), on the host, or left on the device (keep=True)
  lof          the local outlier factor and the local reachability density of every row of a graph (gr_lof_dev)
  overlap      per row, how many neighbours two graphs over the same rows share, and the mean share (gr_knn_overlap_dev)

The arithmetic is stated in include/ganrev.h; everything runs where the table lies.  All pairs are visited: n^2 d work, at most 262144 rows.
"""
import contextlib

import numpy as np

from . import _lib as L
from .nn_utils import DeviceScope, DeviceTensor, deviceTable

MAX_ROWS, MAX_COLUMNS, MAX_K = L.Context.KNN_MAX_N, L.Context.KNN_MAX_D, L.Context.KNN_MAX_K
METRICS = tuple(sorted(L.Context.KNN_METRICS))


class Graph:
    """idx [n x k] int32: row i's k nearest rows j != i by (distance, j) ascending; dist [n x k] float64: their distances; metric as given"""

    def __init__(self, idx, dist, metric=None):
        self.idx, self.dist, self.metric = idx, dist, metric
        self.n, self.k = idx.shape


class DeviceGraph:
    """A Graph where gr_knn_dev left it: idx_dev [n x k] int32, dist_dev [n x k] doubles.  numpy() copies it to the host; close() (or leaving a
    `with` block over it) frees it."""

    def __init__(self, ctx, n, k, metric=None):
        self.ctx, self.n, self.k, self.metric = ctx, int(n), int(k), metric
        self.mem = DeviceScope(ctx)
        self.idx_dev, self.dist_dev = self.mem.malloc(4 * self.n * self.k), self.mem.malloc(8 * self.n * self.k)

    def numpy(self):
        return Graph(self.ctx.download(self.idx_dev, (self.n, self.k), np.int32), self.ctx.download(self.dist_dev, (self.n, self.k), np.float64), self.metric)

    def close(self):
        self.mem.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def checkShape(n, d, k, metric="cosine"):
    if metric not in L.Context.KNN_METRICS:
        raise L.GanrevError(f"knn: metric {metric!r}: one of {sorted(L.Context.KNN_METRICS)}")
    if not 2 <= int(n) <= MAX_ROWS:
        raise L.GanrevError(f"knn: n {n}: 2 to {MAX_ROWS} rows (every pair of rows is visited)")
    if not 1 <= int(d) <= MAX_COLUMNS:
        raise L.GanrevError(f"knn: d {d}: 1 to {MAX_COLUMNS} columns")
    if not 1 <= int(k) <= min(int(n) - 1, MAX_K):
        raise L.GanrevError(f"knn: k {k}: 1 to min(n - 1, {MAX_K}) = {min(int(n) - 1, MAX_K)} neighbours (a row is not its own)")


def graph(ctx, table, k, metric="cosine", rows=None, keep=False):
    """The k-nearest-neighbour graph of `table`: a DeviceTensor [N x d], a (pointer, N, d) triple, or a host array [N x d], uploaded to a temporary
    buffer first as deviceTable does.  rows=M: the graph of the first M rows alone.  -> Graph; keep=True: a DeviceGraph, which the caller closes"""
    if isinstance(table, tuple):
        ptr, N, d = table
        table = DeviceTensor(ctx, (N, d), ptr)                                # a view: the caller keeps the memory
    elif not isinstance(table, DeviceTensor):
        table = np.asarray(table, np.float32)
    if rows is not None and not 0 < int(rows) <= table.shape[0]:
        raise L.GanrevError(f"knn.graph: rows {rows}: the first rows of a table of {table.shape[0]}")
    with deviceTable(ctx, table, rows=None if rows is None else int(rows)) as (ptr, n, d):
        checkShape(n, d, k, metric)
        g = DeviceGraph(ctx, n, k, metric)
        try:
            ctx.knn_dev(ptr, n, d, k, metric, g.idx_dev, g.dist_dev)
            if keep:
                return g
            with g:
                return g.numpy()
        except Exception:
            g.close()
            raise


@contextlib.contextmanager
def _onDevice(ctx, g, distances=True):
    """a Graph or a DeviceGraph -> (idx_dev, dist_dev) for the length of a block"""
    if isinstance(g, DeviceGraph):
        yield g.idx_dev, g.dist_dev
        return
    with DeviceScope(ctx) as own:
        yield (own.upload(np.ascontiguousarray(g.idx, np.int32)), own.upload(np.ascontiguousarray(g.dist, np.float64)) if distances else None)


def lof(ctx, g):
    """-> (lof, lrd) [n] float64 of a Graph or a DeviceGraph: the local outlier factor (about 1 inside a region of even density, larger the
    sparser a row's neighbourhood is against its neighbours') and the local reachability density"""
    with _onDevice(ctx, g) as (idx, dist), DeviceScope(ctx) as own:
        out, lrd = own.malloc(8 * g.n), own.malloc(8 * g.n)
        ctx.lof_dev(idx, dist, g.n, g.k, out, lrd)
        return ctx.download(out, (g.n,), np.float64), ctx.download(lrd, (g.n,), np.float64)


def overlap(ctx, a, b):
    """-> (count [n] int32: the entries of a's row i that are in b's row i; the mean of count / k) of two graphs over the same rows with the same k"""
    if (a.n, a.k) != (b.n, b.k):
        raise L.GanrevError(f"knn.overlap: graphs of {a.n} x {a.k} and {b.n} x {b.k}: the same rows and the same k")
    with _onDevice(ctx, a, False) as (ia, _), _onDevice(ctx, b, False) as (ib, _), DeviceScope(ctx) as own:
        count, mean = own.malloc(4 * a.n), own.malloc(8)
        ctx.knn_overlap_dev(ia, ib, a.n, a.k, count, mean)
        return ctx.download(count, (a.n,), np.int32), float(ctx.download(mean, (1,), np.float64)[0])
