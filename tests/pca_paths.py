"""numpy restatement of gr_pca_dev's and gr_pca_project_dev's summation structure (include/ganrev.h states it; csrc/pca.hip), and the error bounds
that follow from that structure - derived here, not tuned against the device.

Structure.  RPB = 512 rows per block.  Mean: fp64, rows of a block in row order, block partials in block order, one division.  Covariance: the
centred value c = fl32(fl64(x - mean)); per block and element one fp32 chain of L = 512 products (multiply and add rounded separately); P = 128
partial matrices, partial p adding the chains of blocks floor(p B / P) .. floor((p + 1) B / P) - 1 in fp64; the partials added in order in fp64; one
division by n - 1.  Jacobi: fp64, round-robin, stop at off_F <= TAU ||C||_F with TAU = 2^-46 or after SWEEP_CAP = 30 sweeps.  Projection: per
(row, axis) one fp32 chain over the d columns, the whitening one fp64 multiply rounded to fp32 once.

Bounds.  u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64); gamma(k, w) = k w / (1 - k w) bounds (1 + w)^k - 1.
  mean_i        a chain of at most RPB adds, then B adds, one division: gamma(RPB + B + 1, v) mean_r |x_ri|; the float64 reference adds its own
                gamma(n, v) mean_r |x_ri| at worst.
  cov_ij        every product passes the two centring roundings, its own rounding and at most L - 1 adds: (L + 2) u as the issue states it (one to
                spare) plus the centring term 2 u, in all gamma(L + 4, u); the fp64 joins: at most ceil(B / P) adds into a partial, P adds of
                partials, the conversion and the division: c = ceil(B / P) + P + 2 roundings, and the float64 reference's n + 2 more.  All of this
                times S_ij = sum_r |c_ri c_rj| / (n - 1).  Centring at the computed mean m^ = m + delta instead of the reference's adds
                n delta_i delta_j / (n - 1) + (delta_i |sum_r c_rj| + delta_j |sum_r c_ri|) / (n - 1) with delta bounded by the mean's bound.
  eigenvalues   Weyl: the final diagonal is within off_F <= TAU ||C||_F of the final matrix's eigenvalues, and every round of disjoint rotations
                perturbs the matrix by at most 32 v ||C||_F in norm - two 2-term combinations per element (4 v ||A||_F per pass, two passes: 8 v),
                c and s off an exact rotation by at most 4 v (8 v for the two-sided product), the pivot block's closed forms and explicit zero
                16 v.  A sweep has m - 1 rounds (m = d + d mod 2): r(d, sweeps) = 32 (m - 1) sweeps + 4 d, the 4 d for LAPACK's own error in the
                reference and the test's float64 products.
  residual      (TAU + 2 r v) ||C||_F for the fp64 pair (the accumulated V is as far from orthogonal as A is from a similarity), and the fp32
                rounding of the axis moves C v - lambda v by at most (||C||_2 + |lambda|) u <= 2 ||C||_F u.
  orthogonality |V V^T - I| <= 2 r v + 2 u + u^2.
  vectors       Davis-Kahan with ||dC||_2 <= (TAU + r v) ||C||_F: sin(theta_a) <= 2 ||dC||_2 / gap_a; for unit vectors |v - w| = 2 sin(theta / 2) <=
                sqrt(2) sin(theta), and the fp32 rounding of the axis adds u.
  projection    centring rounding, product rounding, at most d - 1 adds, the whitening's one rounding to fp32: gamma(d + 2, u) sum_t |c_t v_t| times the
                whitening scale (the issue's (d + 2) u); the fp64 whitening product and the float64 reference add gamma(d + 6, v).
"""
import math

import numpy as np

RPB, L, P = 512, 512, 128
TAU, SWEEP_CAP = 2.0 ** -46, 30
MAX_D = 256
U32, U64 = 2.0 ** -24, 2.0 ** -53


def gamma(k, w):
    return k * w / (1.0 - k * w)


def blocks(n):
    return -(-n // RPB)


def partial_ranges(n):
    """[(first block, one past the last block)] of the P partial matrices"""
    b = blocks(n)
    return [(p * b // P, (p + 1) * b // P) for p in range(P)]


# ------------------------------------------------------------------ the restatement
def mean(x):
    x = np.asarray(x, np.float32)
    n, d = x.shape
    total = np.zeros(d, np.float64)
    for b in range(blocks(n)):
        s = np.zeros(d, np.float64)
        for r in range(b * RPB, min((b + 1) * RPB, n)):
            s = s + x[r].astype(np.float64)
        total = total + s
    return total / np.float64(n)


def centre(x, mean_):
    return (np.asarray(x, np.float32).astype(np.float64) - np.asarray(mean_, np.float64)).astype(np.float32)


def covariance(x, mean_):
    c = centre(x, mean_)
    n, d = c.shape
    total = np.zeros((d, d), np.float64)
    for lo, hi in partial_ranges(n):
        part = np.zeros((d, d), np.float64)
        for b in range(lo, hi):
            acc = np.zeros((d, d), np.float32)
            for r in range(b * RPB, min((b + 1) * RPB, n)):
                acc = acc + c[r][:, None] * c[r][None, :]           # float32 product, float32 add
            part = part + acc.astype(np.float64)
        total = total + part
    return total / np.float64(n - 1)


def project(x, mean_, axes, eigenvalues, k, whiten):
    c = centre(x, mean_)
    v = np.asarray(axes, np.float32)[:k]
    acc = np.zeros((c.shape[0], k), np.float32)
    for t in range(c.shape[1]):
        acc = acc + c[:, t][:, None] * v[:, t][None, :]
    if not whiten:
        return acc
    ev = np.asarray(eigenvalues, np.float64)[:k]
    pos = ev > 0
    scale = np.where(pos, 1.0 / np.sqrt(np.where(pos, ev, 1.0)), 0.0)
    return np.where(pos[None, :], (acc.astype(np.float64) * scale[None, :]).astype(np.float32), np.float32(0))


# ------------------------------------------------------------------ the bounds
def mean_bound(x, reference_too=True):
    x = np.abs(np.asarray(x, np.float64))
    n = len(x)
    k = RPB + blocks(n) + 1 + (n if reference_too else 0)
    return gamma(k, U64) * x.mean(axis=0)


def cov_fp64_roundings(n):
    return -(-blocks(n) // P) + P + 2


def cov_bound(x):
    """per element, against the float64 two-pass covariance of the same table"""
    x = np.asarray(x, np.float64)
    n = len(x)
    c = x - x.mean(axis=0)
    s = (np.abs(c).T @ np.abs(c)) / (n - 1)
    delta = mean_bound(x)
    drift = np.abs(c.sum(axis=0)) / (n - 1)
    centring = n * np.outer(delta, delta) / (n - 1) + np.outer(delta, drift) + np.outer(drift, delta)
    return (gamma(L + 4, U32) + gamma(cov_fp64_roundings(n) + n + 2, U64)) * s + centring


def rotation_term(d, sweeps):
    m = d + (d & 1)
    return 32 * (m - 1) * sweeps + 4 * d


def eigenvalue_bound(cov, sweeps):
    f = np.linalg.norm(cov)
    return (TAU + rotation_term(len(cov), sweeps) * U64) * f


def residual_bound(cov, sweeps):
    f = np.linalg.norm(cov)
    return (TAU + 2 * rotation_term(len(cov), sweeps) * U64) * f + 2 * f * U32


def orthogonality_bound(d, sweeps):
    return 2 * rotation_term(d, sweeps) * U64 + 2 * U32 + U32 * U32


def vector_bound(cov, sweeps, reference_eigenvalues):
    """per axis: |v_library - (+-) v_reference|_2"""
    w = np.asarray(reference_eigenvalues, np.float64)
    gap = np.full(len(w), np.inf)
    if len(w) > 1:
        dif = np.abs(np.diff(w))
        gap[:-1] = dif
        gap[1:] = np.minimum(gap[1:], dif)
    dc = (TAU + rotation_term(len(cov), sweeps) * U64) * np.linalg.norm(cov)
    return math.sqrt(2.0) * 2.0 * dc / gap + U32


def project_bound(scale_sums, d):
    """scale_sums: pca_oracle.project's T_ra (whitening scale included)"""
    return (gamma(d + 2, U32) + gamma(d + 6, U64)) * np.asarray(scale_sums, np.float64)
