"""A two-dimensional map of the recovered noise: exact t-SNE on the device (no counterpart in the reference; its first result section,
"Embedding learned by G", wants one picture of how the recovered noise is organised - ganrev.pca walks straight axes and the clusters are
disconnected blocks).

  affinities   the joint probabilities P [n x n] of a device table [n x d], n <= 16384 (gr_tsne_affinities_dev)
  embed        P, a starting layout (the first two principal axes, or normal noise) and the optimisation (gr_tsne_run_dev) -> Embedding
  mapCells     the row nearest to the centre of every cell of a grid over the map (gr_map_cells_dev): what gr_image_grid_dev draws

The arithmetic is stated in include/ganrev.h; everything runs where the table lies.  Barnes-Hut, FFT interpolation and sparse affinities are out
of scope: larger corpora are mapped by a prefix of their rows or by their cluster centroids.
"""
import numpy as np

from . import _lib as L
from . import device

INIT_SD = 1e-4                       # standard deviation of the starting layout's first column (the reference implementations start at 1e-4 N(0, 1))


class Affinities:
    """What affinities returns.  Device buffers (one owner, freed by close()): p_dev [n x n] floats, beta_dev [n] doubles.  Downloaded: beta,
    tries (the most updates of beta a row needed), capped (rows that still missed the tolerance after 50)."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        self.mem = device.Buffers(ctx)
        self.p_dev, self.beta_dev, self.info_dev = self.mem.malloc(4 * self.n * self.n), self.mem.malloc(8 * self.n), self.mem.malloc(8)

    def matrix(self):
        return self.ctx.download(self.p_dev, (self.n, self.n))

    def close(self):
        self.mem.close()


class Embedding(Affinities):
    """What embed returns: an Affinities with the map.  Further device buffers: y_dev, inc_dev, gains_dev [n x 2] floats, kl_dev doubles.
    Downloaded: y [n x 2]; kl_iterations and kl (the KL divergence before the first iteration and after every kl_every-th, and after the last);
    eta, perplexity, iterations."""

    def __init__(self, ctx, n, n_kl):
        super().__init__(ctx, n)
        self.y_dev, self.inc_dev, self.gains_dev = (self.mem.malloc(8 * self.n) for _ in range(3))
        self.kl_dev = self.mem.malloc(8 * n_kl)


def _check(n, perplexity):
    if not 4 <= n <= L.Context.TSNE_MAX_N:
        raise L.GanrevError(f"t-SNE: n {n}: 4 to GR_TSNE_MAX_N = {L.Context.TSNE_MAX_N} rows (map a prefix of the rows, or the cluster centroids)")
    if not 1 <= perplexity <= (n - 1) / 3:
        raise L.GanrevError(f"t-SNE: perplexity {perplexity}: 1 to (n - 1) / 3 = {(n - 1) / 3:g}")


def _affinities(a, table_dev, d, perplexity):
    ctx = a.ctx
    ctx.tsne_affinities_dev(table_dev, a.n, d, perplexity, a.p_dev, a.beta_dev, a.info_dev)
    a.beta = ctx.download(a.beta_dev, (a.n,), np.float64)
    info = ctx.download(a.info_dev, (2,), np.int32)
    a.tries, a.capped, a.perplexity = int(info[0]), int(info[1]), float(perplexity)


def affinities(ctx, table_dev, n, d, perplexity):
    """table_dev: pointer of a device table [n x d] floats -> Affinities (the caller closes it)"""
    n, d = int(n), int(d)
    _check(n, perplexity)
    a = Affinities(ctx, n)
    try:
        _affinities(a, table_dev, d, perplexity)
    except Exception:
        a.close()
        raise
    return a


def defaultEta(n, exaggeration=12.0):
    """max(n / exaggeration, 50): bhtsne's fixed 200 oscillates at small n"""
    return max(n / float(exaggeration), 50.0)


def initialLayout(ctx, table_dev, n, d, init="pca", seed=1):
    """[n x 2] float32, first column of standard deviation INIT_SD.  "pca": the coordinates along the first two principal axes (gr_pca_dev,
    gr_pca_project_dev; one axis and a zero column for d = 1; d within gr_pca_dev's limit);
    "random": gr_fill_normal_dev with `seed`."""
    if init == "pca":
        from . import pca as P
        k = min(2, d)
        axes = P.principalAxes(ctx, table_dev, n, d)
        try:
            t = P.project(ctx, axes, table_dev, n, k)
            try:
                y = t.numpy().astype(np.float64)
            finally:
                t.free()
        finally:
            axes.close()
        if k == 1:
            y = np.concatenate([y, np.zeros_like(y)], axis=1)
    elif init == "random":
        buf = ctx.malloc(8 * n)
        try:
            ctx.fill_normal(buf, 2 * n, seed)
            y = ctx.download(buf, (n, 2)).astype(np.float64)
        finally:
            ctx.free(buf)
    else:
        raise L.GanrevError(f"t-SNE: init {init!r}: 'pca' or 'random'")
    sd = y[:, 0].std()
    return (y * (INIT_SD / sd if sd > 0 else 1.0)).astype(np.float32)


def embed(ctx, table_dev, n, d, perplexity=30, iterations=1000, init="pca", seed=1, eta=None, exaggeration=12, stop_lying_iter=250,
          mom_switch_iter=250, kl_every=50, y0=None):
    """The map of the device table [n x d] -> Embedding (the caller closes it).  y0 [n x 2]: a starting layout of the caller's instead of `init`."""
    n, d, iterations, kl_every = int(n), int(d), int(iterations), int(kl_every)
    _check(n, perplexity)
    if iterations < 0 or kl_every < 0:
        raise L.GanrevError("t-SNE: iterations and kl_every must not be negative")
    eta = defaultEta(n, exaggeration) if eta is None else float(eta)
    n_every = iterations // kl_every if kl_every else 0
    e = Embedding(ctx, n, n_every + 2)
    try:
        _affinities(e, table_dev, d, perplexity)
        y = initialLayout(ctx, table_dev, n, d, init, seed) if y0 is None else np.ascontiguousarray(y0, np.float32).reshape(n, 2)
        ctx.upload(y, e.y_dev); ctx.upload(np.zeros((n, 2), np.float32), e.inc_dev); ctx.upload(np.ones((n, 2), np.float32), e.gains_dev)
        e.config = L.TsneConfig(eta, exaggeration, stop_lying_iter, 0.5, 0.8, mom_switch_iter, 0.01)
        ctx.tsne_kl_dev(e.p_dev, e.y_dev, n, e.kl_dev)                                        # slot 0: before the first iteration
        ctx.tsne_run_dev(e.p_dev, n, e.config, e.y_dev, e.inc_dev, e.gains_dev, 0, iterations, e.kl_dev + 8 if kl_every else None, kl_every)
        its = [0] + [kl_every * (i + 1) for i in range(n_every)]
        if its[-1] != iterations:
            ctx.tsne_kl_dev(e.p_dev, e.y_dev, n, e.kl_dev + 8 * len(its))
            its.append(iterations)
        e.kl_iterations, e.kl = its, ctx.download(e.kl_dev, (len(its),), np.float64)
        e.y = ctx.download(e.y_dev, (n, 2))
    except Exception:
        e.close()
        raise
    e.eta, e.iterations = eta, iterations
    return e


def mapCells(ctx, y_dev, n, grid_h, grid_w=None, counts=False):
    """y_dev: pointer of a device layout [n x 2] floats -> rows [grid_h x grid_w] int64, the row nearest to each cell's centre (-1: empty; axis 0
    of the map runs along grid_w); with counts=True also the rows per cell [grid_h x grid_w] int32"""
    grid_h = int(grid_h); grid_w = grid_h if grid_w is None else int(grid_w)
    cells = max(grid_h * grid_w, 1)
    mem = device.Buffers(ctx)
    try:
        rows_dev, counts_dev = mem.malloc(8 * cells), mem.malloc(4 * cells) if counts else None
        ctx.map_cells_dev(y_dev, n, grid_h, grid_w, rows_dev, counts_dev)
        rows = ctx.download(rows_dev, (grid_h, grid_w), np.int64)
        return (rows, ctx.download(counts_dev, (grid_h, grid_w), np.int32)) if counts else rows
    finally:
        mem.close()
