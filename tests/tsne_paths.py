"""The summation structure of csrc/tsne.hip restated in numpy (include/ganrev.h states it), and the error bounds the t-SNE tests assert, each
derived from the kernel's operation chain and evaluated in float64 on the actual operands.  u = 2^-24 (one float32 rounding), v = 2^-53 (one
float64 rounding).  The bounds are first order in u, v and the stop tolerance of the search; every factor (1 + u)^k - 1 is kept as written so
that no constant is picked by hand."""
import numpy as np

import tsne_oracle as to

U, V = 2.0 ** -24, 2.0 ** -53
TINY = 2.0 ** -149                       # the spacing of float32 below 2^-126: a value stored there is within TINY, not within u of itself
RPB = 512                                # rows per block of the column mean (kernels.h ROWS_PER_BLOCK)
MAX_N = 16384


def gamma(k):
    """the relative error of a float64 sum of k terms in any order (k - 1 additions at most along a path), plus one rounding per term"""
    return (k + 1) * V / (1 - (k + 1) * V)


# ------------------------------------------------------------------ affinities
def _row(D, i):
    others = np.arange(len(D)) != i
    return D[i, others], others


def distance_error(D, d):
    """|D_dev - D|: the differences are exact in float64; d squares and d additions each rounded on the device, and the same in the oracle"""
    return 2 * gamma(2 * d) * D


def entropy_eval_bound(D, d, i, beta):
    """|H the device evaluated at beta - H of the float64 distances at beta|.  dH / dr_j = -beta^2 p_j (r_j - E r) (r = D - min); r carries the
    distance error of both operands of the subtraction and the argument error of exp (2 v (beta r) relative to e_j, the same as 2 v r on r); the
    three sums over n - 1 terms and log, the division and the product add gamma(n + 3) of each of H's two terms."""
    row, _ = _row(D, i)
    r = row - row.min()
    _, p = to.entropy(r, beta)
    mean = (p * r).sum()
    dr = distance_error(row, d) + distance_error(row.min(), d) + 4 * V * r
    s = np.exp(-beta * r).sum()
    return float(beta * beta * (p * np.abs(r - mean) * dr).sum() + gamma(len(D) + 3) * (abs(np.log(s)) + 2 * beta * mean + 1))


def conditional_bound(D, d, betas):
    """|c_dev - c| of the conditional matrix: both searches stop within TOL + the evaluation bound of log(perplexity), so their H differ by at
    most twice that; dH / dbeta = -beta Var_p(r) turns it into |beta_dev - beta|, and dc_j / dbeta = -c_j (r_j - E r).  One float32 rounding of
    the stored value (relative u, or TINY where float32 underflows gradually) and the float64 evaluation error gamma(n + 3) come on top.  A row
    whose distances are all equal does not depend on beta."""
    n = len(D)
    out = np.zeros((n, n))
    for i in range(n):
        row, others = _row(D, i)
        r = row - row.min()
        _, p = to.entropy(r, betas[i])
        mean = (p * r).sum()
        var = (p * (r - mean) ** 2).sum()
        dbeta = 2 * (to.TOL + entropy_eval_bound(D, d, i, betas[i])) / (betas[i] * var) if var > 0 else 0.0
        dr = distance_error(row, d) + distance_error(row.min(), d)                     # dc_j / dr_k = -beta c_j ((j == k) - c_k)
        out[i, others] = p * np.abs(r - mean) * dbeta + p * (U + gamma(n + 3) + betas[i] * (dr + (p * dr).sum())) + TINY
    return out


def joint_bound(D, d, betas, P):
    """p_ij = (float)((c_ij + c_ji) / 2n): the two conditional bounds over 2n, one float32 rounding and one float64 addition and division"""
    c = conditional_bound(D, d, betas)
    return (c + c.T) / (2 * len(D)) + (U + 2 * V) * P + TINY


def total_bound(n):
    """|sum p - 1|: every row of c sums to 1 up to one float32 rounding per entry (u in all) and gamma; the symmetrisation rounds once more"""
    return 2 * U + 2 * gamma(n + 3)


# ------------------------------------------------------------------ gradient and KL: the float32 chain up to w, float64 after
def weights32(y):
    """dx = y_i0 - y_j0, dy = y_i1 - y_j1, w = 1 / (1 + (dx dx + dy dy)), every operation rounded to float32 -> (dx, dy, w) as float64"""
    y = np.asarray(y, np.float32)
    dx, dy = y[:, None, 0] - y[None, :, 0], y[:, None, 1] - y[None, :, 1]
    w = np.float32(1) / (np.float32(1) + (dx * dx + dy * dy))
    return dx.astype(np.float64), dy.astype(np.float64), w.astype(np.float64)


EW = (1 + U) ** 6 - 1        # relative error of w: dx (u), its square (2 u + u), the sum (u), 1 + d2 (u) - all damped by d2 / (1 + d2) <= 1 - and the division (u)


def gradient(P, y, exaggeration, drop=None):
    """the library's gradient up to the order of its float64 sums -> (g float32 [n x 2], Z).  drop: "4", "exaggeration" or "w2" leaves that
    factor out (the mutation check)."""
    dx, dy, w = weights32(y)
    P = np.asarray(P, np.float32).astype(np.float64)
    z = w.sum() - np.trace(w)
    e = 1.0 if drop == "exaggeration" else float(np.float32(exaggeration))
    ww = w if drop == "w2" else w * w
    g = np.stack([e * (P * w * dx).sum(axis=1) - (ww * dx).sum(axis=1) / z, e * (P * w * dy).sum(axis=1) - (ww * dy).sum(axis=1) / z], axis=1)
    return ((1.0 if drop == "4" else 4.0) * g).astype(np.float32), z


def gradient_bound(P, y, exaggeration):
    """|g_dev - g| per element.  Attraction e p w dx: w (EW) and dx (u).  Repulsion w^2 dx / Z: w twice, dx, and Z, a sum of positive terms each
    within EW.  The float64 sums: gamma(n + 16) of the absolute terms.  The result is rounded to float32 once."""
    P = np.asarray(P, np.float64)
    n = len(P)
    diff, w = to.weights(y)
    z = w.sum() - n
    g, _ = to.gradient(P, y, exaggeration)
    acc = gamma(n + 16)
    att = exaggeration * ((P * w)[:, :, None] * np.abs(diff)).sum(axis=1)
    rep = ((w * w)[:, :, None] * np.abs(diff)).sum(axis=1) / z
    first = 4.0 * (att * (EW + U + acc) + rep * (3 * EW + U + 2 * acc))
    return first * (1 + U) + U * np.abs(g)


def kl_bound(P, y):
    """|kl_dev - kl|: log w within EW (1 + EW) per entry, log Z within the same; float64 sums and logs: gamma(n + 16) of the absolute terms"""
    P = np.asarray(P, np.float64)
    n = len(P)
    _, w = to.weights(y)
    z = w.sum() - n
    on = P > 0
    rel = EW * (1 + EW)
    return float(2 * rel * P.sum() + gamma(n + 16) * ((P[on] * (np.abs(np.log(P[on])) + np.abs(np.log(w[on])))).sum() + abs(np.log(z)) * P.sum()))


# ------------------------------------------------------------------ update: the bits
def sign(v):
    return (v > 0).astype(np.int8) - (v < 0).astype(np.int8)


def column_mean(y):
    """float64: per block of 512 rows the rows in row order from +0.0, the blocks in block order from +0.0, one division by n"""
    y = np.asarray(y, np.float32).astype(np.float64)
    s = np.zeros(2)
    for b in range(0, len(y), RPB):
        s = s + (np.zeros(2) + np.cumsum(y[b:b + RPB], axis=0)[-1])
    return s / float(len(y))


def update(y, grad, inc, gains, eta, momentum, min_gain):
    """gr_tsne_update_dev in float32 numpy, operation by operation -> (y, inc, gains, y before the re-centring)"""
    f = np.float32
    y, grad, inc, gains = (np.asarray(a, f) for a in (y, grad, inc, gains))
    gains = np.where(sign(grad) == sign(inc), gains * f(0.8), gains + f(0.2)).astype(f)
    gains = np.where(gains < f(min_gain), f(min_gain), gains).astype(f)
    inc = (f(momentum) * inc - (f(eta) * gains) * grad).astype(f)
    moved = (y + inc).astype(f)
    centred = (moved.astype(np.float64) - column_mean(moved)[None, :]).astype(f)
    return centred, inc, gains, moved


def mean_bound(moved, centred):
    """|column mean of the result|: the computed mean is within gamma(n + 2) mean|y| of the mean; every y - mean is rounded to float32 once"""
    n = len(moved)
    return gamma(n + 2) * np.abs(np.asarray(moved, np.float64)).mean(axis=0) + U * np.abs(np.asarray(centred, np.float64)).mean(axis=0)


def schedule(t, exaggeration, stop_lying_iter, mom_switch_iter, momentum=(0.5, 0.8)):
    return (exaggeration if t < stop_lying_iter else 1.0), (momentum[0] if t < mom_switch_iter else momentum[1])


# ------------------------------------------------------------------ cells: the bits
def cells(y, gh, gw):
    """gr_map_cells_dev in float32 numpy -> (rows int64 [gh x gw], counts int32 [gh x gw])"""
    f = np.float32
    y = np.asarray(y, f)
    lo, hi = y.min(axis=0), y.max(axis=0)
    cell, centre = [], []
    for axis, g in ((0, gw), (1, gh)):
        if hi[axis] > lo[axis]:
            t = ((y[:, axis] - lo[axis]) / (hi[axis] - lo[axis])) * f(g)
            c = np.minimum(t.astype(np.int32), g - 1)
        else:
            c = np.zeros(len(y), np.int32)
        cell.append(c)
        centre.append(lo[axis] + (c.astype(f) + f(0.5)) * ((hi[axis] - lo[axis]) / f(g)))
    da, db = y[:, 0] - centre[0], y[:, 1] - centre[1]
    d2 = (da * da + db * db).astype(f)
    rows, counts = np.full(gh * gw, -1, np.int64), np.zeros(gh * gw, np.int32)
    best = np.full(gh * gw, np.inf)
    index = cell[1].astype(np.int64) * gw + cell[0]
    for i in range(len(y)):                                               # ascending rows: a tie keeps the lower one
        c = index[i]
        counts[c] += 1
        if d2[i] < best[c]:
            best[c], rows[c] = d2[i], i
    return rows.reshape(gh, gw), counts.reshape(gh, gw)
