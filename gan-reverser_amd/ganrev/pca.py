"""Principal axes of the recovered noise (no counterpart in the reference; its README asks for another coordinate system twice: "G does not
connect single features with single components", "maybe other clustering methods would produce better results").

  principalAxes    mean, covariance eigenvalues and unit axes of a device table [n x d], d <= 256 (gr_pca_dev)
  project          [n x k] coordinates of the rows along the first k axes, optionally whitened (gr_pca_project_dev)
  axisVariations   the noise rows mean + t * sqrt(eigenvalue) * axis: apply_r.lua:110-136's variations along the axes instead of the coordinates

The arithmetic is stated in include/ganrev.h; everything runs where the table lies.
"""
import numpy as np

from . import _lib as L
from . import device
from .nn_utils import DeviceTensor


class PrincipalAxes:
    """What principalAxes returns.  Device buffers (one owner, freed by close()): mean_dev [d] doubles, cov_dev [d x d] doubles, eigvals_dev [d]
    doubles, axes_dev [d x d] floats.  Downloaded: mean, eigenvalues (descending, as computed: a rank-deficient table may give -tiny), axes
    (row a = unit axis a), explained (each positive eigenvalue over their sum, 0 for the others), sweeps, converged."""

    def __init__(self, ctx, n, d):
        self.ctx, self.n, self.d = ctx, int(n), int(d)
        self.mem = device.Buffers(ctx)
        self.mean_dev, self.cov_dev, self.eigvals_dev = (self.mem.malloc(8 * b) for b in (d, d * d, d))
        self.axes_dev, self.info_dev = self.mem.malloc(4 * d * d), self.mem.malloc(8)

    def covariance(self):
        return self.ctx.download(self.cov_dev, (self.d, self.d), np.float64)

    def close(self):
        self.mem.close()


def explainedRatios(eigenvalues):
    """each positive eigenvalue over the sum of the positive ones (zeros when there is none)"""
    ev = np.asarray(eigenvalues, np.float64)
    pos = np.where(ev > 0, ev, 0.0)
    total = pos.sum()
    return pos / total if total > 0 else pos


def principalAxes(ctx, table_dev, n, d):
    """table_dev: pointer of a device table [n x d] floats (2 <= n < 2^31, d <= 256) -> PrincipalAxes (the caller closes it)"""
    n, d = int(n), int(d)
    if d > ctx.PCA_MAX_D:
        raise L.GanrevError(f"principalAxes: d {d}: at most {ctx.PCA_MAX_D} columns (pixel-space tables are out of scope)")
    p = PrincipalAxes(ctx, n, d)
    try:
        ctx.pca_dev(table_dev, n, d, p.mean_dev, p.cov_dev, p.eigvals_dev, p.axes_dev, p.info_dev)
        p.mean, p.eigenvalues = ctx.download(p.mean_dev, (d,), np.float64), ctx.download(p.eigvals_dev, (d,), np.float64)
        p.axes = ctx.download(p.axes_dev, (d, d))
        info = ctx.download(p.info_dev, (2,), np.int32)
    except Exception:
        p.close()
        raise
    p.sweeps, p.converged = int(info[0]), bool(info[1])
    p.explained = explainedRatios(p.eigenvalues)
    return p


def project(ctx, pca, table_dev, n, k, whiten=False):
    """coordinates of the rows of table_dev [n x pca.d] along the first k axes -> DeviceTensor [n x k] (the caller frees it); whiten divides
    column a by sqrt(eigenvalue a) (a column whose eigenvalue is not positive becomes 0)"""
    n, k = int(n), int(k)
    if not 1 <= k <= pca.d:
        raise L.GanrevError(f"project: k {k}: 1 to {pca.d} axes")
    out = DeviceTensor(ctx, (n, k))
    try:
        ctx.pca_project_dev(table_dev, n, pca.d, pca.mean_dev, pca.axes_dev, pca.eigvals_dev, k, whiten, out.ptr)
    except Exception:
        out.free()
        raise
    return out


def axisVariations(pca, nbAxes, nbSteps=16, noiseMethod="normal"):
    """[nbAxes * nbSteps x d] float32: row a * nbSteps + i = mean + t_i * sqrt(max(eigenvalue a, 0)) * axis a with t = linspace(-3, 3, nbSteps)
    (apply_r.lua:116-122 walks a coordinate the same way); clamped to [-1, 1] for "uniform" noise, the range G was trained on"""
    nbAxes = int(nbAxes)
    if not 1 <= nbAxes <= len(pca.eigenvalues):
        raise L.GanrevError(f"axisVariations: nbAxes {nbAxes}: 1 to {len(pca.eigenvalues)}")
    t = np.linspace(-3, 3, int(nbSteps))
    sd = np.sqrt(np.maximum(np.asarray(pca.eigenvalues, np.float64)[:nbAxes], 0.0))
    rows = np.asarray(pca.mean, np.float64)[None, None, :] + t[None, :, None] * sd[:, None, None] * np.asarray(pca.axes, np.float64)[:nbAxes, None, :]
    rows = rows.reshape(nbAxes * len(t), -1)
    if noiseMethod == "uniform":
        rows = np.clip(rows, -1.0, 1.0)
    return rows.astype(np.float32)
