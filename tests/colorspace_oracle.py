"""numpy oracle of NN_UTILS.switchColorSpace (utils/nn_utils.lua:133-246): the per-pixel formulas include/ganrev.h states for
gr_colorspace_*, written twice - in float32 in the stated operation order (the bit-exact twin of the kernel: every operation
below is one IEEE fp32 operation, none is fused) and in float64 (the yardstick the twin itself is held to).

Images are [N x planes x H x W]; "y" has one plane, "rgb" / "yuv" / "hsl" three.  max / min are compare-selects, as in the kernel.
"""
import numpy as np

SPACES = ("rgb", "y", "yuv", "hsl")          # GR_CS_RGB .. GR_CS_HSL
PLANES = {"rgb": 3, "y": 1, "yuv": 3, "hsl": 3}


def _consts(dt):
    f = dt.type
    return f, f(f(1) / f(3)), f(f(1) / f(6)), f(f(2) / f(3))      # 1/3, 1/6, 2/3 rounded once in the working precision


def _planes(x):
    return x[:, 0], x[:, 1], x[:, 2]


def _stack(*p):
    return np.ascontiguousarray(np.stack(p, axis=1))


def _hue(p, q, t, dt):
    f, _, c16, c23 = _consts(dt)
    t = np.where(t < 0, t + f(1), t)
    t = np.where(t > 1, t - f(1), t)
    a = p + ((q - p) * f(6)) * t
    c = p + ((q - p) * (c23 - t)) * f(6)
    return np.where(t < c16, a, np.where(t < f(0.5), q, np.where(t < c23, c, p))).astype(dt)


def to_rgb(x, from_, dtype=np.float32):
    dt = np.dtype(dtype)
    f, c13, _, _ = _consts(dt)
    x = np.asarray(x, dt)
    if from_ == "rgb":
        return x
    if from_ == "y":
        return np.ascontiguousarray(np.repeat(x, 3, axis=1))
    if from_ == "yuv":
        y, u, v = _planes(x)
        return _stack(y + f(1.13983) * v, (y - f(0.39465) * u) - f(0.58060) * v, y + f(2.03211) * u)
    if from_ == "hsl":
        h, s, l = _planes(x)
        with np.errstate(all="ignore"):
            q = np.where(l < f(0.5), l * (f(1) + s), (l + s) - l * s)
            p = f(2) * l - q
            r, g, b = _hue(p, q, h + c13, dt), _hue(p, q, h, dt), _hue(p, q, h - c13, dt)
        gray = s == 0
        return _stack(np.where(gray, l, r), np.where(gray, l, g), np.where(gray, l, b)).astype(dt)
    raise ValueError(from_)


def from_rgb(x, to, dtype=np.float32):
    dt = np.dtype(dtype)
    f = dt.type
    x = np.asarray(x, dt)
    if to == "rgb":
        return x
    r, g, b = _planes(x)
    z = np.zeros_like(r)
    if to == "y":
        return np.ascontiguousarray((((z + f(0.21) * r) + f(0.72) * g) + f(0.07) * b)[:, None])
    if to == "yuv":
        return _stack(((z + f(0.299) * r) + f(0.587) * g) + f(0.114) * b,
                      ((z - f(0.14713) * r) - f(0.28886) * g) + f(0.436) * b,
                      ((z + f(0.615) * r) - f(0.51499) * g) - f(0.10001) * b)
    if to == "hsl":
        mx = np.where(r > g, r, g); mx = np.where(mx > b, mx, b)
        mn = np.where(r < g, r, g); mn = np.where(mn < b, mn, b)
        with np.errstate(all="ignore"):
            d = mx - mn
            l = (mx + mn) / f(2)
            s = np.where(l > f(0.5), d / ((f(2) - mx) - mn), d / (mx + mn))
            h = np.where(mx == r, (g - b) / d + np.where(g < b, f(6), f(0)),
                         np.where(mx == g, (b - r) / d + f(2), (r - g) / d + f(4))) / f(6)
        gray = mx == mn
        return _stack(np.where(gray, f(0), h), np.where(gray, f(0), s), np.where(gray, mx, l)).astype(dt)
    raise ValueError(to)


def switch(x, from_, to, dtype=np.float32):
    """toRgb(from) then rgbToColorSpace(to) (utils/nn_utils.lua:133-137); y -> y, yuv -> yuv and hsl -> hsl go through rgb too"""
    out = from_rgb(to_rgb(x, from_, dtype), to, dtype)
    assert out.dtype == np.dtype(dtype)
    return out


def make_images(shape, from_, seed):
    """[N x planes(from_) x H x W] float32 test input for the bit-exact comparisons: uniform [0, 1], then a block of exact grays,
    exact two-way ties, 0 / 1 saturated pixels, and values outside [0, 1] (yuv's negative chroma; out-of-gamut rgb; a hue that wraps).
    No NaN can arise from finite inputs here: the only divisions are by d = mx - mn (non-zero past the gray test), by mx + mn and by
    2 - mx - mn, so a zero divisor gives an infinity, never 0 / 0.  No -0.0 is put in either."""
    n, h, w = shape
    c = PLANES[from_]
    rng = np.random.default_rng(seed)
    x = rng.random((n, c, h, w), dtype=np.float32)
    flat = x.transpose(0, 2, 3, 1).reshape(-1, c)           # a copy: one row per pixel
    m = flat.shape[0]
    k = max(1, m // 8)
    if c == 3:
        flat[0:k] = flat[0:k, :1]                           # exact grays (hsl input: h = s = l; rgb: mx == mn)
        flat[k:2 * k, 1] = flat[k:2 * k, 0]                 # ties between the first two planes (mx == r == g or mn == r == g)
        flat[2 * k:3 * k, 2] = flat[2 * k:3 * k, 1]         # ties between the last two
        sat = rng.integers(0, 2, (k, c)).astype(np.float32)
        flat[3 * k:4 * k] = sat                             # every 0 / 1 corner of the cube, many times
        if from_ == "yuv":
            flat[4 * k:5 * k, 1:] = rng.uniform(-0.6, 0.6, (k, 2)).astype(np.float32)      # signed chroma
        elif from_ == "rgb":
            flat[4 * k:5 * k] = rng.uniform(0.05, 1.3, (k, c)).astype(np.float32)          # out of gamut, above 1
        else:
            flat[4 * k:5 * k, 0] = rng.uniform(-0.5, 1.5, k).astype(np.float32)            # hue outside [0, 1]: one wrap
            flat[5 * k:6 * k, 1] = 0                                                      # s == 0: the gray branch
    else:
        flat[0:k] = rng.integers(0, 2, (k, 1)).astype(np.float32)
        flat[k:2 * k] = rng.uniform(-0.25, 1.25, (k, 1)).astype(np.float32)
    return np.ascontiguousarray(flat.reshape(n, h, w, c).transpose(0, 3, 1, 2))
