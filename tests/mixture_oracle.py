"""float64 numpy reference of gr_mixture_dev (include/ganrev.h): a diagonal-covariance Gaussian mixture fitted by EM, with the rules of the
library - a component with N_j < 1 keeps its mean and variances, the variance floor, the first maximum as the label - and the inputs of the tests."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


def log_density(x, weights, means, variances):
    """l [n, k] = log w_j - (d log 2 pi + sum_t log var_jt) / 2 - sum_t (x_it - mu_jt)^2 / (2 var_jt); -inf for w_j = 0"""
    x, w = np.asarray(x, np.float64), np.asarray(weights, np.float64)
    mu, var = np.asarray(means, np.float64), np.asarray(variances, np.float64)
    d = x.shape[1]
    with np.errstate(divide="ignore"):
        c = np.log(w) - 0.5 * (d * LOG_2PI + np.log(var).sum(axis=1))
    q = np.empty((len(x), len(w)))
    for j in range(len(w)):
        q[:, j] = (((x - mu[j]) ** 2) * (0.5 / var[j])).sum(axis=1)
    return c[None, :] - q


def e_step(x, weights, means, variances):
    """-> dict(l [n, k], rowll [n], r [n, k], labels [n], post [n], loglik)"""
    l = log_density(x, weights, means, variances)
    m = l.max(axis=1)
    with np.errstate(invalid="ignore"):
        s = np.exp(l - m[:, None]).sum(axis=1)
        rowll = m + np.log(s)
        r = np.exp(l - rowll[:, None])
    labels = l.argmax(axis=1)                                           # numpy's argmax: the first maximum
    return dict(l=l, rowll=rowll, r=r, labels=labels, post=r[np.arange(len(l)), labels], loglik=float(rowll.mean()))


def m_step(x, r, weights, means, variances, var_floor):
    """-> (weights', means', variances'): the second moment about the old mean; N_j < 1 keeps mean and variances"""
    x, r = np.asarray(x, np.float64), np.asarray(r, np.float64)
    mu, var = np.array(means, np.float64), np.array(variances, np.float64)
    n = len(x)
    big_n = r.sum(axis=0)
    for j in range(len(big_n)):
        if big_n[j] >= 1.0:
            new = (r[:, j, None] * x).sum(axis=0) / big_n[j]
            second = (r[:, j, None] * (x - mu[j]) ** 2).sum(axis=0) / big_n[j]
            var[j] = np.maximum(second - (new - mu[j]) ** 2, var_floor)
            mu[j] = new
    return big_n / n, mu, var


def fit(x, weights, means, variances, iterations, var_floor):
    """-> (weights, means, variances, loglik [iterations + 1], the last E-step)"""
    w, mu, var = np.asarray(weights, np.float64), np.asarray(means, np.float64), np.asarray(variances, np.float64)
    hist = []
    for _ in range(iterations):
        e = e_step(x, w, mu, var)
        hist.append(e["loglik"])
        w, mu, var = m_step(x, e["r"], w, mu, var, var_floor)
    e = e_step(x, w, mu, var)
    hist.append(e["loglik"])
    return w, mu, var, np.array(hist), e


# ------------------------------------------------------------------ inputs
def blobs(n, d, k, seed=0, separation=6.0):
    """k unit-variance blobs [n, d] float32 whose centres are `separation` apart from each other at least along one column, rows in random order;
    -> (x, centres [k, d] float32)"""
    rng = np.random.default_rng(seed + 1000 * n + d)
    centres = rng.standard_normal((k, d))
    centres[:, 0] = separation * np.arange(k)                           # 6 sigma apart along column 0, whatever the other columns hold
    which = rng.permutation(np.arange(n) % k)                           # every blob has floor(n / k) rows at least
    x = centres[which] + rng.standard_normal((n, d))
    return x.astype(np.float32), centres.astype(np.float32)


def start(x, means0):
    """the initial parameters ganrev.mixture.fit uses: weights 1 / k, the table's column variances (n - 1 in the divisor) for every component"""
    x = np.asarray(x, np.float32)
    k = len(means0)
    var = x.astype(np.float64).var(axis=0, ddof=1) if len(x) > 1 else np.ones(x.shape[1])
    return np.full(k, 1.0 / k, np.float32), np.asarray(means0, np.float32), np.tile(var.astype(np.float32), (k, 1))


def spread_start(x, k, seed=0):
    """parameters a few EM steps away from a fit, as floats: means near distinct rows, unequal weights, unequal variances"""
    x = np.asarray(x, np.float32)
    rng = np.random.default_rng(seed + 7 * k)
    n, d = x.shape
    means = x[rng.integers(0, n, k)].astype(np.float64) + 0.1 * rng.standard_normal((k, d))
    w = rng.uniform(0.5, 1.5, k)
    var = rng.uniform(0.5, 2.0, (k, d))
    return (w / w.sum()).astype(np.float32), means.astype(np.float32), var.astype(np.float32)
