"""float64 numpy yardstick of gr_pca_dev / gr_pca_project_dev (include/ganrev.h), and the tables the PCA tests share.  The reference has no PCA
and oracle/ none either: plain numpy is the reference here.  one_pass_f32 is the formula the library must NOT use (E[xx^T] - mean mean^T in
float32): the tests assert that it misses the stated bound where the corpus sits far from the origin, so that case is known to bite."""
import functools

import numpy as np

from ganrev import synth


def mean(x):
    return np.asarray(x, np.float64).mean(axis=0)


def centred(x):
    x = np.asarray(x, np.float64)
    return x - x.mean(axis=0)


def covariance(x):
    """two-pass, centred, float64: 1 / (n - 1) sum_r c_r c_r^T"""
    c = centred(x)
    return (c.T @ c) / (len(c) - 1)


def abs_product_sums(x):
    """S_ij = sum_r |c_ri c_rj| / (n - 1): the scale of the covariance bound"""
    c = np.abs(centred(x))
    return (c.T @ c) / (len(c) - 1)


def one_pass_f32(x):
    """E[xx^T] - mean mean^T with float32 accumulators (row by row), scaled by n / (n - 1): what a one-pass kernel would compute"""
    x = np.asarray(x, np.float32)
    n, d = x.shape
    s1, s2 = np.zeros(d, np.float32), np.zeros((d, d), np.float32)
    for r in range(n):
        s1 = s1 + x[r]
        s2 = s2 + x[r][:, None] * x[r][None, :]
    m = s1 / np.float32(n)
    return ((s2 / np.float32(n) - m[:, None] * m[None, :]) * np.float32(n / (n - 1))).astype(np.float64)


def eigh_descending(cov):
    """np.linalg.eigh of a float64 matrix -> (eigenvalues descending, axes [d x d] with row a = eigenvector a)"""
    w, v = np.linalg.eigh(np.asarray(cov, np.float64))
    order = np.argsort(-w, kind="stable")
    return w[order], v[:, order].T.copy()


def sign_rule_holds(axes):
    """every row's largest-magnitude component, the first among equals, is positive"""
    a = np.asarray(axes)
    first = np.argmax(np.abs(a), axis=1)                # argmax returns the first maximum
    return bool((a[np.arange(len(a)), first] > 0).all())


def project(x, mean_, axes, eigenvalues, k, whiten):
    """float64: (x - mean) . axes[:k]^T, column a over sqrt(eigenvalue a) when whiten (0 where the eigenvalue is not positive); also returns
    T_ra = sum_t |c_rt v_at| (times the whitening scale): the scale of the projection bound.  The centred value is the library's, rounded to
    float32 once; its rounding is part of the bound, so the reference keeps the float64 difference."""
    c = np.asarray(x, np.float64) - np.asarray(mean_, np.float64)
    v = np.asarray(axes, np.float64)[:k]
    out, scale_sum = c @ v.T, np.abs(c) @ np.abs(v.T)
    if whiten:
        ev = np.asarray(eigenvalues, np.float64)[:k]
        s = np.where(ev > 0, 1.0 / np.sqrt(np.where(ev > 0, ev, 1.0)), 0.0)
        out, scale_sum = out * s, scale_sum * s
    return out, scale_sum


# ------------------------------------------------------------------ tables (computed once, shared, never written to)
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def gaussian(n, d, seed=3):
    """correlated normal columns, about unit scale, off the origin by a fraction"""
    z = synth.normal((n, d), seed).astype(np.float64)
    mix = synth.normal((d, d), seed + 1).astype(np.float64) / np.sqrt(d)
    off = synth.uniform((d,), seed + 2).astype(np.float64)
    return _frozen((z @ mix + off).astype(np.float32))


@functools.lru_cache(maxsize=None)
def far_from_origin(n, d, seed=5):
    """mean 1000 and standard deviation 1 per column"""
    return _frozen((1000.0 + synth.normal((n, d), seed).astype(np.float64)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def geometric_spectrum(n, d, ratio=0.9, seed=7):
    """normal rows scaled to variances ratio^a along the axes of a random rotation: every gap of the spectrum is large"""
    q, _ = np.linalg.qr(synth.normal((d, d), seed).astype(np.float64))
    z = synth.normal((n, d), seed + 1).astype(np.float64) * np.sqrt(ratio ** np.arange(d))
    return _frozen((z @ q.T).astype(np.float32))


@functools.lru_cache(maxsize=None)
def isotropic(n, d, seed=9):
    return _frozen(synth.normal((n, d), seed).astype(np.float32))


@functools.lru_cache(maxsize=None)
def with_constant_column(n, d, column=2, seed=11):
    x = np.array(gaussian(n, d, seed))
    x[:, column] = 0.75
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def independent_columns(d, seed=13):
    """a symmetric table whose covariance is exactly diagonal in float arithmetic: rows +e_t s_t and -e_t s_t"""
    s = (1.0 + np.arange(d)[::-1]).astype(np.float32)
    x = np.zeros((2 * d, d), np.float32)
    x[np.arange(d), np.arange(d)] = s
    x[d + np.arange(d), np.arange(d)] = -s
    return _frozen(x)
