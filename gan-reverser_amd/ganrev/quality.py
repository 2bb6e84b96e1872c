"""Image-to-image scores of a reconstruction: the structural similarity index (SSIM, Wang et al. 2004) and PSNR beside the plain squared error.

L2 rewards blur, and regression to the mean is what the reference's README names as the fix-faces loop's artefact: a structural score is what tells a
sharp wrong face from a smooth average one.  ssim() scores two image tables where they lie (gr_ssim_dev, csrc/quality.hip); reconstruct() is
G(R(x)) on the device; ssim_twin() restates the kernel's operation chain (include/ganrev.h) in numpy for the tests that run without a GPU.

The defaults are the usual ones: an 11 x 11 Gaussian window of sigma 1.5 over the valid positions, data_range 1 (every G here ends in nn.Sigmoid).
"""
import math

import numpy as np

from . import _lib as L
from .nn_utils import DeviceTensor, forwardBatchedDev

WIN, SIGMA, DATA_RANGE = 11, 1.5, 1.0
ROWS_PER_BLOCK = 512        # the unit of the mean's chain (include/ganrev.h)


def check_tables(a, b):
    """(n, channels, h, w) of two image tables of one shape, or an error"""
    if len(a.shape) != 4 or tuple(a.shape) != tuple(b.shape):
        raise L.GanrevError(f"ssim: a {tuple(a.shape)} / b {tuple(b.shape)} are not two tables [n x channels x h x w] of one shape")
    return tuple(int(v) for v in a.shape)


def ssim(a, b, win=WIN, sigma=SIGMA, data_range=DATA_RANGE):
    """SSIM and mean squared error per image of two DeviceTensors [N x C x H x W] -> (ssim_rows [N] float32, mse_rows [N] float32, the mean SSIM):
    one gr_ssim_dev; the tables stay where they are and 8 N + 8 bytes come back."""
    n, c, h, w = check_tables(a, b)
    L.ssim_check_args(n, c, h, w, win, data_range)
    ctx = a.ctx
    rows, mse, mean = DeviceTensor(ctx, (n,)), DeviceTensor(ctx, (n,)), ctx.malloc(8)
    try:
        ctx.ssim_dev(a.ptr, b.ptr, n, c, h, w, rows.ptr, mse.ptr, mean, win=win, sigma=sigma, data_range=data_range)
        return rows.numpy(), mse.numpy(), float(ctx.download(mean, (1,), np.float64)[0])
    finally:
        rows.free(); mse.free(); ctx.free(mean)


def psnr(mse_rows, data_range=DATA_RANGE):
    """10 log10(L^2 / mse) per row in float64, inf where the error is 0"""
    mse = np.asarray(mse_rows, np.float64)
    out = np.full(mse.shape, np.inf)
    pos = mse > 0
    out[pos] = 10.0 * np.log10(float(data_range) ** 2 / mse[pos])
    return out


def reconstruct(model_g, model_r, images, batchSize):
    """G(R(x)) for a DeviceTensor of images [N x C x H x W], both nets in evaluate() mode, in chunks of batchSize -> a DeviceTensor of the same
    shape (the caller frees it).  The image table never visits the host."""
    ctx = images.ctx
    model_g.evaluate(); model_r.evaluate()
    rnet = model_r.device_net(images.shape[1:])
    if ctx.conv_mode() == "f16x3":
        rnet.range_guard_scan()           # the *_dev calls are not range-guarded (include/ganrev.h): one synchronous scan per net, as in embed_dev
    z = forwardBatchedDev(model_r, images, batchSize)
    try:
        if ctx.conv_mode() == "f16x3":
            model_g.device_net(z.shape[1:]).range_guard_scan()
        out = forwardBatchedDev(model_g, z, batchSize)
    finally:
        z.free()
    if tuple(out.shape) != tuple(images.shape):
        shape = out.shape; out.free()
        raise L.GanrevError(f"reconstruct: G gives {shape[1:]}, the images are {images.shape[1:]}")
    return out


def score_summary(values):
    """mean / median / 5 % / 95 % of a score, as compare's summary.json holds them (inf stays inf: Python's json writes Infinity)"""
    v = np.asarray(values, np.float64)
    return dict(mean=float(v.mean()), median=float(np.median(v)), p05=float(np.percentile(v, 5)), p95=float(np.percentile(v, 95)))


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's chain in numpy (include/ganrev.h, "image-to-image scores"): same operations, same order, one rounding each.  numpy's elementwise
# operations round on their own, like the kernel's (compiled without FMA contraction).  dtype = np.float32 runs the same chain in single precision:
# what the tests use to show that their bounds tell the two apart.
def window(win, sigma):
    """g[0 .. win) in float64: the Gaussian exp(-(d d) / (2 sigma sigma)), d = i - (win - 1) / 2, over its sum in index order; sigma <= 0: 1 / win"""
    if sigma <= 0:
        return np.full(win, 1.0 / float(win))
    mid, den = float(win - 1) / 2.0, 2.0 * (float(sigma) * float(sigma))
    e = [math.exp(-((float(i) - mid) * (float(i) - mid)) / den) for i in range(win)]
    s = 0.0
    for v in e:
        s = s + v
    return np.array([v / s for v in e], np.float64)


def _ordered_sum(x, axis):
    """the slices of x along `axis` added in index order from +0.0"""
    x = np.moveaxis(x, axis, 0)
    s = np.zeros(x.shape[1:], x.dtype)
    for v in x:
        s = s + v
    return s


def ssim_twin(a, b, win=WIN, sigma=SIGMA, data_range=DATA_RANGE, dtype=np.float64):
    """gr_ssim_dev's chain on host arrays [N x C x H x W] -> (ssim_rows float32, mse_rows float32, mean).  Needs no GPU."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, c, h, w = check_tables(a, b)
    L.ssim_check_args(n, c, h, w, win, data_range)
    T = np.dtype(dtype).type
    g = window(win, sigma).astype(dtype)
    k1, k2 = 0.01 * float(data_range), 0.03 * float(data_range)
    c1, c2 = T(k1 * k1), T(k2 * k2)
    x, y = a.astype(dtype), b.astype(dtype)
    ow, oh = w - win + 1, h - win + 1

    def passes(q):
        hq = np.zeros(q.shape[:3] + (ow,), dtype)
        for t in range(win):
            hq = hq + g[t] * q[..., t:t + ow]
        v = np.zeros(q.shape[:2] + (oh, ow), dtype)
        for t in range(win):
            v = v + g[t] * hq[:, :, t:t + oh, :]
        return v
    mx, my, sxx, syy, sxy = passes(x), passes(y), passes(x * x), passes(y * y), passes(x * y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    vx, vy, cxy = sxx - mxx, syy - myy, sxy - mxy
    n1 = T(2.0) * mxy + c1
    n2 = T(2.0) * cxy + c2
    d1 = (mxx + myy) + c1
    d2 = (vx + vy) + c2
    s = (n1 * n2) / (d1 * d2)
    per_image = lambda e: _ordered_sum(_ordered_sum(_ordered_sum(e, 3), 2), 1)         # columns, rows, channels
    q = per_image(s) / T(c * oh * ow)
    d = x - y
    m = per_image(d * d) / T(c * h * w)
    parts = [_ordered_sum(q[lo:lo + ROWS_PER_BLOCK], 0) for lo in range(0, n, ROWS_PER_BLOCK)]
    mean = _ordered_sum(np.array(parts, dtype), 0) / T(n)
    return q.astype(np.float32), m.astype(np.float32), float(mean)
