"""Float64 reference of the structural similarity index in the DIRECT form - independent of the kernel's separable sum w x^2 - mu^2 form:
the full 2-D window at every valid position, the centred moments sum w (x - mu_x)^2 and sum w (x - mu_x)(y - mu_y), np.mean over positions and
channels.  Also the image kinds and the shapes the SSIM tests share (the issue's list), and one cached reference per case."""
import functools

import numpy as np

# (n, C, h, w, win)
SHAPES = [(1, 1, 3, 3, 3), (2, 1, 11, 11, 11),                       # one valid position each
          (3, 3, 11, 12, 11), (3, 1, 5, 9, 3), (2, 3, 33, 17, 7),    # odd, non-square, w % 4 != 0
          (4, 3, 32, 32, 11), (2, 3, 64, 64, 11), (1, 1, 128, 128, 11),   # ... the cap
          (513, 1, 11, 11, 11), (1025, 1, 3, 3, 3)]                  # the row mean's 512-row block edges
KINDS = ["noise", "negative", "constants", "black_white", "cancellation"]


def window2d(win, sigma):
    if sigma <= 0:
        return np.full((win, win), 1.0 / (win * win))
    i = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    g = g / g.sum()
    return np.outer(g, g)


def patches(x, win):
    """[n, C, oh, ow, win, win] view of every valid window of a float64 table"""
    return np.lib.stride_tricks.sliding_window_view(x, (win, win), axis=(2, 3))


def moments(a, b, win, sigma):
    """per valid position and channel: (mu_x, mu_y, var_x, var_y, cov) in float64, the second moments centred"""
    x, y = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    w2 = window2d(win, sigma)
    px, py = patches(x, win), patches(y, win)
    mx, my = (px * w2).sum(axis=(4, 5)), (py * w2).sum(axis=(4, 5))
    dx, dy = px - mx[..., None, None], py - my[..., None, None]
    vx, vy, cxy = (w2 * dx * dx).sum(axis=(4, 5)), (w2 * dy * dy).sum(axis=(4, 5)), (w2 * dx * dy).sum(axis=(4, 5))
    return mx, my, vx, vy, cxy


def ssim_map(mx, my, vx, vy, cxy, data_range):
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim(a, b, win=11, sigma=1.5, data_range=1.0):
    """-> (ssim_rows [n] float64, mse_rows [n] float64, mean)"""
    mx, my, vx, vy, cxy = moments(a, b, win, sigma)
    rows = np.mean(ssim_map(mx, my, vx, vy, cxy, data_range), axis=(1, 2, 3))
    d = np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)
    return rows, np.mean(d * d, axis=(1, 2, 3)), float(np.mean(rows))


def make_pair(kind, shape, seed=0):
    """(a, b) float32 [n x C x h x w] in [0, 1] of one of the image kinds"""
    n, c, h, w = shape[:4]
    rng = np.random.default_rng(1000 * seed + 17 * KINDS.index(kind) + n + 3 * h + 5 * w)
    dims = (n, c, h, w)
    if kind == "noise":                      # b = a + N(0, 0.05^2), clipped
        a = rng.random(dims)
        b = np.clip(a + rng.normal(0.0, 0.05, dims), 0.0, 1.0)
    elif kind == "negative":                 # b = 1 - a: negative SSIM
        a = rng.random(dims)
        b = 1.0 - a
    elif kind == "constants":                # two different constants per image: sigma = 0 on both sides
        a = np.broadcast_to(rng.random((n, 1, 1, 1)), dims)
        b = np.broadcast_to(rng.random((n, 1, 1, 1)), dims)
    elif kind == "black_white":              # SSIM ~ C1 / (1 + C1)
        a, b = np.zeros(dims), np.ones(dims)
    elif kind == "cancellation":             # bright, low contrast: var = sum w x^2 - mu^2 cancels
        a = 0.9 + 0.1 * rng.random(dims)
        b = np.clip(a + rng.normal(0.0, 1e-3, dims), 0.0, 1.0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


@functools.lru_cache(maxsize=None)
def case(kind, shape, sigma=1.5, data_range=1.0):
    """the pair, the reference and the bounds of one case, computed once and shared (read-only arrays)"""
    import ssim_paths
    a, b = make_pair(kind, shape)
    win = shape[4]
    ref = ssim(a, b, win, sigma, data_range)
    bounds = ssim_paths.bounds(a, b, win, sigma, data_range)
    for arr in (a, b) + ref[:2]:
        arr.setflags(write=False)
    return a, b, ref, bounds
