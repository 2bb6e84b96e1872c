"""Silhouette coefficients of a clustering of the recovered noise, on the device (no counterpart in the reference; its README closes the
clustering section with "the similarity is rather low ... maybe other clustering methods would produce better results" - this is the number
that says whether one did).  For a row i in cluster A: a = the mean distance to the other rows of A, b = the smallest mean distance to the rows
of another cluster, s = (b - a) / max(a, b), between -1 (in the wrong cluster) and 1 (well inside its own).  It needs no truth labels, only the
table and the labelling, so the k-means labels, --closest, the whitened projection and the mixture's labels are all scored by the same rule.

  score        every row's s, a, b and nearest other cluster, the per-cluster means, the sizes and the mean (gr_silhouette_dev)

The arithmetic is stated in include/ganrev.h; everything runs where the table lies.  All pairs are visited: n^2 d work, at most 262144 rows.
"""
import numpy as np

from . import _lib as L
from .nn_utils import DeviceTensor, deviceTable

MAX_ROWS = L.Context.SILHOUETTE_MAX_N


class Silhouette:
    """values, a, b [n] float64, nearest [n] int32 (-1: no other cluster has a member, or the row has no cluster), cluster_mean [k] float64
    (0 for an empty cluster), sizes [k] int32, mean: the mean of values over all n rows (rows without a cluster count as 0); metric as given"""

    def __init__(self, values, a, b, nearest, cluster_mean, sizes, mean, metric):
        self.values, self.a, self.b, self.nearest = values, a, b, nearest
        self.cluster_mean, self.sizes, self.mean, self.metric = cluster_mean, sizes, float(mean), metric
        self.n, self.k = len(values), len(sizes)

    def summary(self):
        """what a summary.json keeps: the mean, the per-cluster means and the sizes"""
        return dict(mean=self.mean, cluster_mean=[float(v) for v in self.cluster_mean], sizes=[int(v) for v in self.sizes])


def checkShape(n, d, k, metric="cosine"):
    C = L.Context
    if metric not in C.SILHOUETTE_METRICS:
        raise L.GanrevError(f"silhouette: metric {metric!r}: one of {sorted(C.SILHOUETTE_METRICS)}")
    if not 2 <= int(n) <= C.SILHOUETTE_MAX_N:
        raise L.GanrevError(f"silhouette: n {n}: 2 to {C.SILHOUETTE_MAX_N} rows (every pair of rows is visited)")
    if not 1 <= int(d) <= C.SILHOUETTE_MAX_D:
        raise L.GanrevError(f"silhouette: d {d}: 1 to {C.SILHOUETTE_MAX_D} columns")
    if not 1 <= int(k) <= C.SILHOUETTE_MAX_K:
        raise L.GanrevError(f"silhouette: k {k}: 1 to {C.SILHOUETTE_MAX_K} clusters")


def score(ctx, table, labels, k, metric="cosine", rows=None):
    """The silhouette of the labelling `labels` [n] (host integers; a label outside [0, k) belongs to no cluster) of `table`: a DeviceTensor
    [N x d], a (pointer, N, d) triple, or a host array [N x d], uploaded to a temporary buffer first as deviceTable does.  rows=M: the first M
    rows only (labels [M]).  -> Silhouette"""
    labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
    if isinstance(table, tuple):
        ptr, N, d = table
        table = DeviceTensor(ctx, (N, d), ptr)                                # a view: the caller keeps the memory
    n = len(labels) if rows is None else int(rows)
    with deviceTable(ctx, table, rows=n) as (ptr, n_table, d):
        if n != len(labels) or n > n_table:
            raise L.GanrevError(f"silhouette.score: {len(labels)} labels for {n} of the table's {n_table} rows")
        checkShape(n, d, k, metric)
        bufs = []
        try:
            bufs.append(ctx.upload(labels))
            bufs += [ctx.malloc(b) for b in (8 * n, 8 * n, 8 * n, 4 * n, 8 * k, 4 * k, 8)]
            lab, sv, a, b, near, cmean, sizes, mean = bufs
            ctx.silhouette_dev(ptr, n, d, lab, k, metric, sv, cmean, sizes, mean, a, b, near)
            return Silhouette(ctx.download(sv, (n,), np.float64), ctx.download(a, (n,), np.float64), ctx.download(b, (n,), np.float64),
                              ctx.download(near, (n,), np.int32), ctx.download(cmean, (k,), np.float64), ctx.download(sizes, (k,), np.int32),
                              ctx.download(mean, (1,), np.float64)[0], metric)
        finally:
            for p in bufs:
                ctx.free(p)
