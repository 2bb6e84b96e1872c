"""Error bounds of gr_ssim_dev (csrc/quality.hip) and of its numpy twin (ganrev.quality.ssim_twin) against tests/ssim_oracle.py, derived from the
operation chain include/ganrev.h states - not tuned against the device.

u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64); gamma(k) = k v / (1 - k v) bounds (1 + v)^k - 1.  Every fp64 bound is two-sided: the library's
distance from the exact value plus the float64 reference's.  The float outputs are compared with the reference's fp64 value, so their one rounding
counts once: u (|ref| + fp64 bound).  The bounds are running error bounds, evaluated per window position on the reference's own moments.

  window    arg[i] = -(d d) / (2 sigma sigma): d and d d are exact, the denominator and the division one rounding each, so exp sees an argument
            off by 2 v |arg| and moves by that much relatively; exp itself is within 1 ulp = 2 v (glibc and numpy both document less):
            own[i] = 2 + 2 |arg[i]| units of v on e[i] - larger at the far taps, which weigh little.  E = the e[i] added in order: its relative
            error is at most the g-weighted mean of own[] plus win - 1 adds; g = e / E one more: KN = sum_i g[i] own[i] + win units that every tap
            shares.  The uniform window 1 / win: own = 0, KN = 1.
  sums      the library: V = sum_tv g sum_th g q, q exact (a float, or the product of two).  A term passes two weights, one product and at most
            win - 1 adds per tier: |V' - V| <= gamma(2 KN + 2 win) A + v B, A = sum w2 |q|, B = sum w2 (own[i] + own[j]) |q| (the terms of second
            order in v are below 1e-13 of these: the factor 1.001).
            the reference: w2 = g g' one more rounding, the product w2 q, a sum of win^2 terms (any order: gamma(win^2)):
            gamma(2 KN + 2 + win^2) A + v B.
  moments   the library: mxx = mx mx, vx = sxx - mxx - the cancellation: its error is e(sxx) + e(mxx), absolute, whatever is left of vx.
            the reference: centred.  dx = x - mu one rounding; sum w2 dx dx: four more roundings a term, relative to vx, with the tap errors at
            most OWN = 2 max own; a perturbed mean moves a centred moment by its square only.  The covariance likewise, with
            sum w2 |dx| |dy| <= (vx + vy) / 2.
  position  n1, n2, d1, d2, their products and the division: one rounding each (_mul / _add below), C1 and C2 two roundings each on the host.
  image     the library adds ow S in a row, oh rows, C channels and divides: gamma(ow + oh + C + 1) mean |S|; the reference's np.mean over
            three axes: at most gamma(C oh + ow + 2) mean |S|.
  mse       d = x - y one rounding, d d one: gamma(3); the sums as above over h x w.
  mean      the mean of the rows' fp64 bounds, plus blocks of 512, the block chain and one division: gamma(512 + ceil(n / 512) + 1) mean |q|;
            np.mean of n rows: gamma(n + 1).

The cap: with pixels in [0, 1] and data_range 1 the fp64 part may not exceed CAP = 1e-10 on any test case - a float implementation of the window
sums is off by 4.5e-5 on a flat bright image, and a bound that loose would hide it.
"""
import numpy as np

import ssim_oracle as so

U32, U64 = 2.0 ** -24, 2.0 ** -53
TINY32 = 2.0 ** -150
RPB = 512
CAP = 1e-10
SECOND_ORDER = 1.001


def gamma(k):
    return k * U64 / (1.0 - k * U64)


def window_units(win, sigma):
    """(own [win], KN): the units of v on each tap's own exp, and those every tap shares through the normalisation"""
    if sigma <= 0:
        return np.zeros(win), 1.0
    d = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    arg = (d * d) / (2.0 * sigma * sigma)
    own = 2.0 + 2.0 * arg
    g = np.exp(-arg)
    g = g / g.sum()
    return own, float((g * own).sum()) + win


def _mul(a, ea, b, eb):
    """error of fl(a' b') against a b, |a' - a| <= ea, |b' - b| <= eb"""
    t = np.abs(a) * eb + np.abs(b) * ea + ea * eb
    return t + U64 * (np.abs(a * b) + t)


def _add(s, *errs):
    """error of fl(a' + b' ...) against the exact sum s (one rounding per add)"""
    t = sum(errs)
    return t + (len(errs) - 1) * U64 * (np.abs(s) + t)


def _tail(mx, my, vx, vy, cxy, e_mxx, e_myy, e_mxy, e_vx, e_vy, e_cxy, c1, c2):
    """n1 .. S from the moments' errors -> (the error of S, S)"""
    n1, n2 = 2.0 * mx * my + c1, 2.0 * cxy + c2
    d1, d2 = mx * mx + my * my + c1, vx + vy + c2
    e_n1 = _add(n1, 2.0 * e_mxy, 3.0 * U64 * c1)
    e_n2 = _add(n2, 2.0 * e_cxy, 3.0 * U64 * c2)
    e_d1 = _add(d1, e_mxx, e_myy, 3.0 * U64 * c1)
    e_d2 = _add(d2, e_vx, e_vy, 3.0 * U64 * c2)
    e_n, e_d = _mul(n1, e_n1, n2, e_n2), _mul(d1, e_d1, d2, e_d2)
    num, den = n1 * n2, d1 * d2
    s = num / den
    t = (e_n + np.abs(s) * e_d) / (np.abs(den) - e_d)
    return t + U64 * (np.abs(s) + t), s


def position_bounds(a, b, win, sigma, data_range):
    """-> (library side, reference side, S) per valid position and channel"""
    mx, my, vx, vy, cxy = so.moments(a, b, win, sigma)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    own, kn = window_units(win, sigma)
    w2 = so.window2d(win, sigma)
    w2own = w2 * (own[:, None] + own[None, :])
    x, y = np.asarray(a, np.float64), np.asarray(b, np.float64)
    px, py = so.patches(x, win), so.patches(y, win)

    def sums(q, k):                                 # the error of a window sum of q whose shared roundings number k
        q = np.abs(q)
        return SECOND_ORDER * (gamma(k) * (w2 * q).sum(axis=(4, 5)) + U64 * (w2own * q).sum(axis=(4, 5)))
    k1, k2 = 2 * kn + 2 * win, 2 * kn + 2 + win * win
    # the library: second moments minus squares
    e_mx, e_my = sums(px, k1), sums(py, k1)
    e_mxx, e_myy, e_mxy = _mul(mx, e_mx, mx, e_mx), _mul(my, e_my, my, e_my), _mul(mx, e_mx, my, e_my)
    e_vx = _add(vx, sums(px * px, k1), e_mxx)
    e_vy = _add(vy, sums(py * py, k1), e_myy)
    e_cxy = _add(cxy, sums(px * py, k1), e_mxy)
    lib, s = _tail(mx, my, vx, vy, cxy, e_mxx, e_myy, e_mxy, e_vx, e_vy, e_cxy, c1, c2)
    # the reference: centred moments
    r_mx, r_my = sums(px, k2), sums(py, k2)
    r_mxx, r_myy, r_mxy = _mul(mx, r_mx, mx, r_mx), _mul(my, r_my, my, r_my), _mul(mx, r_mx, my, r_my)
    kc = gamma(k2 + 4 + 2 * float(own.max())) * SECOND_ORDER
    r_vx = kc * vx + 4.0 * r_mx * r_mx
    r_vy = kc * vy + 4.0 * r_my * r_my
    r_cxy = kc * 0.5 * (vx + vy) + 4.0 * r_mx * r_my
    ref, _ = _tail(mx, my, vx, vy, cxy, r_mxx, r_myy, r_mxy, r_vx, r_vy, r_cxy, c1, c2)
    return lib, ref, s


def _as_float(ref64, b):
    return b + U32 * (np.abs(ref64) + b) + TINY32


def bounds(a, b, win, sigma=1.5, data_range=1.0):
    """-> dict: rows64 / mse64 / mean64 the fp64 parts (two-sided), rows / mse the bounds of the float outputs against the reference's fp64 values,
    mean the bound of the fp64 mean"""
    n, c, h, w = a.shape
    ow, oh = w - win + 1, h - win + 1
    lib, ref, s = position_bounds(a, b, win, sigma, data_range)
    sabs = np.abs(s).mean(axis=(1, 2, 3))
    rows64 = (lib + ref).mean(axis=(1, 2, 3)) + (gamma(ow + oh + c + 1) + gamma(c * oh + ow + 2)) * sabs
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    mse = np.mean(d * d, axis=(1, 2, 3))
    mse64 = (gamma(3 + w + h + c + 1) + gamma(3 + c * h + w + 2)) * mse
    q = s.mean(axis=(1, 2, 3))
    mean64 = float(rows64.mean()) + (gamma(RPB + -(-n // RPB) + 1) + gamma(n + 1)) * float(np.abs(q).mean())
    return dict(rows64=rows64, mse64=mse64, mean64=mean64, rows=_as_float(q, rows64), mse=_as_float(mse, mse64), mean=mean64)


def ratios(got, ref, bnd):
    """worst err / bound of (ssim_rows, mse_rows, mean) against the reference -> dict; an output that was not asked for is None"""
    rows, mse, mean = got
    out = dict(rows=float(np.max(np.abs(np.asarray(rows, np.float64) - ref[0]) / bnd["rows"])))
    if mse is not None:
        out["mse"] = float(np.max(np.abs(np.asarray(mse, np.float64) - ref[1]) / bnd["mse"]))
    if mean is not None:
        out["mean"] = abs(float(mean) - ref[2]) / bnd["mean"]
    return out
