"""A diagonal-covariance Gaussian mixture of the recovered noise, fitted by EM on the device (no counterpart in the reference; its README closes
the clustering section with "maybe other clustering methods would produce better results").  Where k-means gives every cluster a Voronoi cell,
the mixture gives it a spread of its own, every row a soft membership, and every row a log-likelihood that ranks it from typical to outlying -
an anomaly score in the space the search and the clusters live in.

  fit          EM from given means (the k-means centroids): weights 1 / k, every component's variances the table's column variances (gr_mixture_dev)
  score        labels, posterior at the label and row log-likelihood of any rows under a fitted mixture (gr_mixture_dev with no iteration)
  members      per component the rows of highest posterior, by the member-list kernels of the clustering (gr_cluster_members_wide_dev)

The arithmetic is stated in include/ganrev.h; everything runs where the table lies.
"""
import numpy as np

from . import _lib as L

VAR_FLOOR_FACTOR = 1e-3         # var_floor = this x the mean column variance: a convention (see fit), not a measurement


class Mixture:
    """weights [k], means [k x d], variances [k x d] float32; loglik [iterations + 1] float64, the mean row log-likelihood before every M-step and
    under the final parameters; var_floor as used"""

    def __init__(self, weights, means, variances, loglik, var_floor):
        self.weights, self.means, self.variances = (np.ascontiguousarray(a, np.float32) for a in (weights, means, variances))
        self.loglik, self.var_floor = np.asarray(loglik, np.float64), float(var_floor)
        self.k, self.d = self.means.shape


def checkShape(d, k):
    if not 1 <= int(k) <= L.Context.MIXTURE_MAX_K:
        raise L.GanrevError(f"mixture: k {k}: 1 to {L.Context.MIXTURE_MAX_K} components")
    if not 1 <= int(d) <= L.Context.MIXTURE_MAX_D:
        raise L.GanrevError(f"mixture: d {d}: 1 to {L.Context.MIXTURE_MAX_D} columns")


def columnVariances(ctx, table_dev, n, d):
    """the diagonal of gr_pca_dev's covariance of the device table [n x d] (n - 1 in the divisor) -> [d] float64"""
    from . import pca as P
    axes = P.principalAxes(ctx, table_dev, n, d)
    try:
        return np.diag(axes.covariance()).copy()
    finally:
        axes.close()


def _run(ctx, table_dev, n, d, weights, means, variances, iterations, var_floor, per_row):
    k = len(weights)
    bufs = []
    try:
        for a in (weights, means, variances):
            bufs.append(ctx.upload(np.ascontiguousarray(a, np.float32)))
        bufs.append(ctx.malloc(8 * (iterations + 1)))
        if per_row:
            bufs += [ctx.malloc(4 * n) for _ in range(3)]
        w, mu, var, ll = bufs[:4]
        lab, post, rowll = bufs[4:] if per_row else (None, None, None)
        ctx.mixture_dev(table_dev, n, d, k, iterations, var_floor, w, mu, var, ll, lab, post, rowll)
        fitted = Mixture(ctx.download(w, (k,)), ctx.download(mu, (k, d)), ctx.download(var, (k, d)), ctx.download(ll, (iterations + 1,), np.float64), var_floor)
        rows = (ctx.download(lab, (n,), np.int32), ctx.download(post, (n,)), ctx.download(rowll, (n,))) if per_row else None
        return fitted, rows
    finally:
        for b in bufs:
            ctx.free(b)


def fit(ctx, table_dev, n, d, means0, iterations, var_floor=None, column_variances=None):
    """EM on the device table [n x d] (pointer) from the means means0 [k x d] - the clustering step's final centroids - for `iterations`
    iterations -> Mixture.  Initial weights 1 / k; initial variances, for every component, the table's column variances: the diagonal of
    gr_pca_dev's covariance, taken from column_variances [d] when the caller has it already (--pca computed it); a column whose variance is
    below var_floor (a constant column) starts at var_floor, as it would end.
    var_floor defaults to 1e-3 x the mean column variance.  That factor is a convention - small against any spread the table shows, large
    against rounding - not a measured optimum; pass var_floor to choose another."""
    n, d = int(n), int(d)
    means0 = np.ascontiguousarray(means0, np.float32)
    k = len(means0)
    checkShape(d, k)
    if means0.shape != (k, d):
        raise L.GanrevError(f"mixture.fit: means0 {means0.shape}: [k x {d}]")
    if int(iterations) < 0:
        raise L.GanrevError(f"mixture.fit: iterations {iterations}: an iteration count")
    cv = np.asarray(column_variances if column_variances is not None else columnVariances(ctx, table_dev, n, d), np.float64)
    if var_floor is None:
        var_floor = VAR_FLOOR_FACTOR * float(cv.mean())
    var_floor = float(np.float32(var_floor))
    if not var_floor > 0:
        raise L.GanrevError(f"mixture.fit: var_floor {var_floor:g}: positive (a constant table has no spread to fit)")
    variances0 = np.tile(np.maximum(cv, var_floor).astype(np.float32), (k, 1))
    fitted, _ = _run(ctx, table_dev, n, d, np.full(k, 1.0 / k, np.float32), means0, variances0, int(iterations), var_floor, per_row=False)
    return fitted


def score(ctx, mixture, table_dev, n):
    """rows of a device table [n x mixture.d] under the fitted mixture -> (labels int32 [n], the first maximum of the component log-densities;
    post float32 [n], the responsibility at the label; rowll float32 [n], the row log-likelihood).  The table may be any rows of the fit's space:
    the corpus, or needles from outside it."""
    _, rows = _run(ctx, table_dev, int(n), mixture.d, mixture.weights, mixture.means, mixture.variances, 0, mixture.var_floor, per_row=True)
    return rows


def members(ctx, labels, post, k, m):
    """per component j < k the min(m, rows) rows with that label of highest posterior, descending, ties by row: the clustering's rule for
    similarities -> list of k lists of (row, posterior)"""
    labels, post = np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(post, np.float32)
    n = len(labels)
    bufs = []
    try:
        bufs += [ctx.upload(labels), ctx.upload(post)]
        bufs += [ctx.malloc(b) for b in (8 * k * m, 4 * k * m, 4 * k, 4 * k)]
        lab, sim, rows, rsim, kept, sizes = bufs
        ctx.cluster_members_wide_dev(lab, sim, n, k, m, rows, rsim, kept, sizes)
        hrows, hsim, hkept = ctx.download(rows, (k, m), np.int64), ctx.download(rsim, (k, m)), ctx.download(kept, (k,), np.int32)
    finally:
        for b in bufs:
            ctx.free(b)
    return [[(int(r), float(v)) for r, v in zip(hrows[j, :hkept[j]], hsim[j, :hkept[j]])] for j in range(k)]
