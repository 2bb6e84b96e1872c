"""numpy restatement of gr_mixture_dev's operation chains (include/ganrev.h states them; csrc/mixture.hip), and the error bounds that follow from
those chains - derived here, not tuned against the device.

Structure.  Everything past the loads is fp64, one rounding per operation.  Per component h = 0.5 / var and c = log w - 0.5 (d log 2 pi + S), S the
log var added in column order.  Per (row, component) one chain in column order: dl = x - mu, e = dl dl, q = q + e h; l = c - q.  The components form
GROUPS = 4 contiguous ranges of ceil(k / 4); inside a range the running pair (m, s) is rescaled whenever a larger l arrives; the ranges are joined as
S = sum_g s_g exp(m_g - M), L = M + log S.  RPB = 512 rows per block: the L of a block in row order, the blocks in block order, one division by n.
M-step: r = exp(l - L); per block and (j, t) the chains a1 = a1 + r x, a2 = a2 + r (x - mu)^2, an = an + r in row order; P = 128 partial sets, set p
adding the chains of blocks floor(p B / P) .. floor((p + 1) B / P) - 1, the sets added in order; mu' = S1 / N, var' = max(S2 / N - (mu' - mu)^2,
floor), w' = N / n, mean and variance rounded to float once, and kept when N < 1.

Bounds.  u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64); gamma(k, w) = k w / (1 - k w) bounds (1 + w)^k - 1.  FN = 3: exp and log are taken to be
within 3 ulp = 6 v relative, the limit OpenCL sets for double precision (the device library and glibc both document less).  Every bound below is
two-sided: the library's distance from the exact value plus the float64 reference's, which runs chains no longer than the library's.
  l_ij     the term e h carries the rounding of dl twice (it is squared), of e, of h and of the product, then at most d - 1 adds: gamma(d + 4, v) q.
           c: log w within 6 v |log w|; each log var within 6 v, d - 1 adds; the product d log 2 pi and its constant 2 v; one add, one subtraction:
           gamma(d + 10, v) C_j with C_j = |log w_j| + (d log 2 pi + sum_t |log var_jt|) / 2.  The subtraction c - q: one more rounding of
           at most C_j + q.  One side: gamma(d + 11, v) (C_j + q_ij).
  L_i      arguments that move by at most b_j move log-sum-exp by at most log sum_j r_ij exp(b_ij) = log1p(sum_j r_ij expm1(b_ij)): the upper side
           is the definition; the lower side follows from (sum r e^-b)(sum r e^b) >= (sum r)^2 = 1.  A far component's large bound counts with its
           vanishing responsibility.  Its own arithmetic: a term exp(l_j - M) reaches S
           through at most ceil(k / 4) + 1 rescalings or adds inside its range, one product and at most GROUPS adds in the join.  Every step that
           leaves a term above the underflow threshold has an argument of magnitude below ARG = 746, rounded to within ARG v, an exp within 6 v, a
           product and an add: (ARG + 8) v per step, so S is relatively within gamma((ARG + 8)(ceil(k / 4) + GROUPS + 1), v); log S <= log k adds
           6 v log k, the sum M + log S adds v |L|.  (A term below the underflow threshold is below 2^-1074 of S >= 1: under every other term here.)
  rowll    L rounded to float: + u |L|.
  loglik   the mean of the per-row bounds, plus gamma(RPB + B + 1, v) mean |L| for the library's adds and division and gamma(n + 1, v) for numpy's.
  post     exp(M - L): the argument is within bound(l at the label) + bound(L) + 2 v |M - L|; the result within post (expm1(that) + 12 v), and u post
           for the rounding to float.
  r_ij     the same with l_ij: rho_ij = expm1(bound(l_ij) + bound(L_i) + 2 v |l_ij - L_i|) + 12 v, relative.
  S1, S2, N  a product, at most RPB adds in the block, ceil(B / P) in the set, P across the sets: g = gamma(RPB + ceil(B / P) + P + 1, v), and
           gamma(n + 1, v) for numpy's sum; S2's factor (x - mu)^2 carries 3 more roundings on either side.  |dS1_jt| <= sum_i r_ij (rho_ij + g')
           |x_it| and likewise for S2 (terms (x - mu)^2) and N (terms 1).
  mu'      (dS1 + |mu'| dN) / (N - dN) + 2 v |mu'| for the two divisions; the rounding to float adds u (|mu'| + that).
  var'     S2 / N: (dS2 + (S2 / N) dN) / (N - dN) + 2 v S2 / N; dm = mu' - mu within the fp64 part of mu's bound + 2 v |dm|; dm^2 within
           2 |dm| ddm + ddm^2 + 2 v dm^2; the subtraction 2 v (S2 / N + dm^2); max(., floor) moves nothing further; the rounding to float u (var' + that).
  w'       dN / n + 2 v w' + u w'.
"""
import math

import numpy as np

import mixture_oracle as mo

RPB, P, GROUPS = 512, 128, 4
MAX_D = MAX_K = 256
U32, U64 = 2.0 ** -24, 2.0 ** -53
FN = 3                      # ulp of exp and log: OpenCL's limit for double precision
ARG = 746.0                 # |argument| below which exp stays above the smallest denormal


def gamma(k, w):
    return k * w / (1.0 - k * w)


def blocks(n):
    return -(-n // RPB)


def partial_ranges(n):
    b = blocks(n)
    return [(p * b // P, (p + 1) * b // P) for p in range(P)]


# ------------------------------------------------------------------ the restatement
def log_density(x, weights, means, variances):
    x = np.asarray(x, np.float32).astype(np.float64)
    w, mu, var = (np.asarray(a, np.float32).astype(np.float64) for a in (weights, means, variances))
    n, d = x.shape
    k = len(w)
    h = 0.5 / var
    s = np.zeros(k)
    for t in range(d):
        s = s + np.log(var[:, t])
    with np.errstate(divide="ignore"):
        c = np.log(w) - 0.5 * (d * mo.LOG_2PI + s)
    q = np.zeros((n, k))
    for t in range(d):
        dl = x[:, t, None] - mu[None, :, t]
        e = dl * dl
        q = q + e * h[None, :, t]
    return c[None, :] - q


def e_step(x, weights, means, variances):
    """-> dict(l, rowll (float64, before the rounding to float), labels, post (float64), loglik)"""
    l = log_density(x, weights, means, variances)
    n, k = l.shape
    kq = -(-k // GROUPS)
    ms, ss, bis = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(GROUPS):
            m, s, bi = np.full(n, -np.inf), np.zeros(n), np.full(n, -1)
            for j in range(g * kq, min(k, (g + 1) * kq)):
                lj = l[:, j]
                up = lj > m
                add = ~up & (lj > -np.inf)
                s = np.where(up, s * np.exp(m - lj) + 1.0, np.where(add, s + np.exp(lj - m), s))
                bi = np.where(up, j, bi)
                m = np.where(up, lj, m)
            ms.append(m); ss.append(s); bis.append(bi)
        big_m, idx = np.full(n, -np.inf), np.full(n, -1)
        for g in range(GROUPS):
            up = (bis[g] >= 0) & (ms[g] > big_m)
            big_m, idx = np.where(up, ms[g], big_m), np.where(up, bis[g], idx)
        big_s = np.zeros(n)
        for g in range(GROUPS):
            big_s = np.where(bis[g] >= 0, big_s + ss[g] * np.exp(ms[g] - big_m), big_s)
        rowll = big_m + np.log(big_s)
        post = np.exp(big_m - rowll)
    total = 0.0
    for b in range(blocks(n)):
        s = 0.0
        for i in range(b * RPB, min((b + 1) * RPB, n)):
            s = s + rowll[i]
        total = total + s
    return dict(l=l, rowll=rowll, labels=np.where(idx < 0, 0, idx), post=post, loglik=total / float(n))


def m_step(x, weights, means, variances, var_floor):
    """one M-step after the E-step under the same parameters -> (weights', means', variances') as floats"""
    xf = np.asarray(x, np.float32).astype(np.float64)
    mu, var = np.asarray(means, np.float32), np.asarray(variances, np.float32)
    e = e_step(x, weights, means, variances)
    with np.errstate(invalid="ignore"):
        r = np.where(e["l"] > -np.inf, np.exp(e["l"] - e["rowll"][:, None]), 0.0)
    n, d = xf.shape
    k = r.shape[1]
    mu64 = mu.astype(np.float64)
    s1, s2, sn = np.zeros((k, d)), np.zeros((k, d)), np.zeros(k)
    for lo, hi in partial_ranges(n):
        p1, p2, pn = np.zeros((k, d)), np.zeros((k, d)), np.zeros(k)
        for b in range(lo, hi):
            a1, a2, an = np.zeros((k, d)), np.zeros((k, d)), np.zeros(k)
            for i in range(b * RPB, min((b + 1) * RPB, n)):
                a1 = a1 + r[i][:, None] * xf[i][None, :]
                dl = xf[i][None, :] - mu64
                a2 = a2 + r[i][:, None] * (dl * dl)
                an = an + r[i]
            p1, p2, pn = p1 + a1, p2 + a2, pn + an
        s1, s2, sn = s1 + p1, s2 + p2, sn + pn
    new_mu, new_var = mu.copy(), var.copy()
    fl = float(np.float32(var_floor))
    for j in range(k):
        if sn[j] >= 1.0:
            mn = s1[j] / sn[j]
            dm = mn - mu64[j]
            v = s2[j] / sn[j] - dm * dm
            new_mu[j] = mn.astype(np.float32)
            new_var[j] = np.where(v > fl, v, fl).astype(np.float32)
    return (sn / float(n)).astype(np.float32), new_mu, new_var


# ------------------------------------------------------------------ the bounds (two-sided: library and float64 reference)
def _parts(x, weights, means, variances):
    x, w = np.asarray(x, np.float64), np.asarray(weights, np.float64)
    mu, var = np.asarray(means, np.float64), np.asarray(variances, np.float64)
    d = x.shape[1]
    with np.errstate(divide="ignore"):
        big_c = np.abs(np.log(w)) + 0.5 * (d * mo.LOG_2PI + np.abs(np.log(var)).sum(axis=1))
    q = np.stack([(((x - mu[j]) ** 2) * (0.5 / var[j])).sum(axis=1) for j in range(len(w))], axis=1)
    return big_c, q


def ell_bound(x, weights, means, variances):
    """[n, k]; 0 for a dead component, whose l is -inf on both sides"""
    big_c, q = _parts(x, weights, means, variances)
    d = np.asarray(x).shape[1]
    with np.errstate(invalid="ignore"):
        b = 2.0 * gamma(d + 11, U64) * (big_c[None, :] + q)
    return np.where(np.isfinite(b), b, 0.0)


def rowll_bound(e, lb, as_float=True):
    """e: mixture_oracle.e_step's result, lb: ell_bound -> [n]"""
    k = e["l"].shape[1]
    steps = -(-k // GROUPS) + GROUPS + 1
    own = gamma((ARG + 2 * FN + 2) * steps, U64) + 2 * FN * U64 * math.log(k)
    moved = np.log1p((e["r"] * np.expm1(lb)).sum(axis=1))
    b = moved + 2.0 * (own + U64 * np.abs(e["rowll"]))
    return b + (U32 * (np.abs(e["rowll"]) + b) if as_float else 0.0)


def loglik_bound(e, lb):
    n = len(e["rowll"])
    mean_abs = float(np.abs(e["rowll"]).mean())
    return float(rowll_bound(e, lb, as_float=False).mean()) + (gamma(RPB + blocks(n) + 1, U64) + gamma(n + 1, U64)) * mean_abs


def resp_rel_bound(e, lb):
    """rho [n, k]: relative bound on r_ij"""
    bl = rowll_bound(e, lb, as_float=False)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(e["l"]), np.abs(e["l"] - e["rowll"][:, None]), 0.0)
    return np.expm1(lb + bl[:, None] + 2 * U64 * gap) + 4 * FN * U64


def post_bound(e, lb):
    rho = resp_rel_bound(e, lb)
    rows = np.arange(len(e["labels"]))
    b = e["post"] * rho[rows, e["labels"]]
    return b + U32 * (e["post"] + b)


def decided_rows(e, lb):
    """rows whose label no rounding can change: the float64 log-density at the label exceeds every other component's by more than the two
    bounds on l together (twice the bound, pair by pair)"""
    l = e["l"]
    rows = np.arange(len(l))
    top, btop = l[rows, e["labels"]], lb[rows, e["labels"]]
    with np.errstate(invalid="ignore"):
        margin = top[:, None] - l - (btop[:, None] + lb)
    margin[rows, e["labels"]] = np.inf
    margin = np.where(np.isneginf(l), np.inf, margin)                   # a dead component is dead on both sides
    return margin.min(axis=1) > 0


def m_step_bounds(x, e, lb, means, var_floor):
    """-> dict(weights [k], means [k, d], variances [k, d], alive [k], big_n [k], big_n_bound [k]): bounds on one M-step's float outputs against
    mixture_oracle.m_step.  They hold where both sides take the same side of N_j >= 1: the caller checks |N_j - 1| > big_n_bound."""
    x, mu = np.asarray(x, np.float64), np.asarray(means, np.float64)
    n, d = x.shape
    r = e["r"]
    rho = resp_rel_bound(e, lb)
    g = gamma(RPB + -(-blocks(n) // P) + P + 1, U64) + gamma(n + 1, U64)
    g2 = g + 2 * gamma(3, U64)
    tiny = n * 2.0 ** -1022                                             # responsibilities that underflowed on one side only
    big_n = r.sum(axis=0)
    dn = (r * (rho + g)).sum(axis=0) + tiny
    ds1 = (r * (rho + g)).T @ np.abs(x) + tiny * np.abs(x).max()
    s2 = np.stack([(r[:, j, None] * (x - mu[j]) ** 2).sum(axis=0) for j in range(r.shape[1])])
    ds2 = np.stack([((r[:, j] * (rho[:, j] + g2))[:, None] * (x - mu[j]) ** 2).sum(axis=0) for j in range(r.shape[1])]) + tiny * (np.abs(x).max() + np.abs(mu).max()) ** 2
    alive = big_n >= 1.0
    den = np.where(alive, big_n - dn, 1.0)[:, None]
    safe_n = np.where(alive, big_n, 1.0)[:, None]
    new = (r.T @ x) / safe_n
    dmu64 = (ds1 + np.abs(new) * dn[:, None]) / den + 2 * U64 * np.abs(new)
    second = s2 / safe_n
    dsecond = (ds2 + second * dn[:, None]) / den + 2 * U64 * second
    dm = new - mu
    ddm = dmu64 + 2 * U64 * np.abs(dm)
    dsq = 2 * np.abs(dm) * ddm + ddm * ddm + 2 * U64 * dm * dm
    dvar64 = dsecond + dsq + 2 * U64 * (second + dm * dm)
    var = np.maximum(second - dm * dm, var_floor)
    w = big_n / n
    return dict(weights=dn / n + 2 * U64 * w + U32 * (w + dn / n),
                means=np.where(alive[:, None], dmu64 + U32 * (np.abs(new) + dmu64), 0.0),
                variances=np.where(alive[:, None], dvar64 + U32 * (var + dvar64), 0.0), alive=alive, big_n=big_n, big_n_bound=dn)
