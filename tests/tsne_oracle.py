"""Exact t-SNE in float64 numpy: the definition gr_tsne_*_dev (csrc/tsne.hip) is measured against.  Nothing here restates the library's
summation order - tests/tsne_paths.py does that and derives the bounds."""
import numpy as np

TOL, MAX_TRIES = 1e-5, 50


# ------------------------------------------------------------------ data
def gaussian(n, d, seed=0):
    return np.random.default_rng([n, d, seed]).standard_normal((n, d)).astype(np.float32)


def far_from_origin(n, d, seed=0):
    """mean 1000, sd 1: the case the |x|^2 + |y|^2 - 2xy form loses"""
    return (1000.0 + np.random.default_rng([n, d, seed, 7]).standard_normal((n, d))).astype(np.float32)


def with_duplicates(n, d, seed=0):
    x = gaussian(n, d, seed)
    x[1] = x[0]; x[n // 2] = x[0]; x[n - 1] = x[n - 2]
    return x


def blobs(n, d, c, seed=0):
    """c well-separated Gaussian blobs: centres N(0, 6^2) per coordinate, unit noise -> (x float32 [n x d], labels).  Well-separated is a
    property of the draw, so it is enforced on the draw: the centres are drawn again until every two are at least 2 (sqrt(d) + 3) apart - a
    unit-noise cloud in d dimensions lies within sqrt(d) + 3 of its centre (the radius is chi-distributed: mean below sqrt(d), sd below 1), so
    the clouds do not touch.  (At d = 3 some two of four N(0, 6^2) centres fall closer than that in four draws out of five; at d = 32 never.)"""
    rng = np.random.default_rng([n, d, c, seed])
    while True:
        centres = 6.0 * rng.standard_normal((c, d))
        gaps = np.linalg.norm(centres[:, None, :] - centres[None, :, :], axis=2)[~np.eye(c, dtype=bool)]
        if gaps.min() >= 2 * (np.sqrt(d) + 3):
            break
    labels = np.arange(n) % c
    return (centres[labels] + rng.standard_normal((n, d))).astype(np.float32), labels


def layout(n, scale, seed=0):
    """a layout at a given scale: 1e-4 is the start of a run, 1 the middle, 50 the spread end"""
    return (scale * np.random.default_rng([n, seed, 11]).standard_normal((n, 2))).astype(np.float32)


def random_joint(n, seed=0):
    """a symmetric float32 matrix with a zero diagonal, a third of its entries zero, summing to 1 within rounding: what the gradient reads"""
    rng = np.random.default_rng([n, seed, 3])
    a = rng.random((n, n)) ** 4 * (rng.random((n, n)) > 1 / 3)
    a = np.triu(a, 1)
    a = a + a.T
    return (a / a.sum()).astype(np.float32)


# ------------------------------------------------------------------ affinities
def distances(x):
    """D_ij = sum_k (x_ik - x_jk)^2 from the differences, float64"""
    x = np.asarray(x, np.float64)
    out = np.empty((len(x), len(x)))
    for i in range(len(x)):
        t = x - x[i]
        out[i] = np.einsum("jk,jk->j", t, t)
    return out


def one_pass_distances_f32(x):
    """|x|^2 + |y|^2 - 2xy in float32: what the library must not do"""
    x = np.asarray(x, np.float32)
    sq = (x * x).sum(axis=1, dtype=np.float32)
    return np.maximum(sq[:, None] + sq[None, :] - np.float32(2) * (x @ x.T), np.float32(0)).astype(np.float64)


def entropy(r, beta):
    """H and the conditional distribution of one row; r = D_ij - min_j D_ij over j != i"""
    e = np.exp(-beta * r)
    s = e.sum()
    return np.log(s) + beta * (r * e).sum() / s, e / s


def search(r, log_u):
    """van der Maaten's bisection on beta -> (beta, updates)"""
    beta, lo, hi, tries = 1.0, None, None, 0
    while True:
        diff = entropy(r, beta)[0] - log_u
        if abs(diff) <= TOL or tries == MAX_TRIES:
            return beta, tries
        if diff > 0:
            lo = beta
            beta = beta * 2 if hi is None else (beta + hi) / 2
        else:
            hi = beta
            beta = beta / 2 if lo is None else (beta + lo) / 2
        tries += 1


def conditional(D, betas):
    n = len(D)
    c = np.zeros((n, n))
    for i in range(n):
        others = np.arange(n) != i
        r = D[i, others] - D[i, others].min()
        c[i, others] = entropy(r, betas[i])[1]
    return c


def joint_from_distances(D, perplexity):
    """-> (P float64 [n x n], betas, updates per row)"""
    n = len(D)
    betas, tries = np.empty(n), np.empty(n, np.int64)
    for i in range(n):
        others = np.arange(n) != i
        betas[i], tries[i] = search(D[i, others] - D[i, others].min(), np.log(perplexity))
    c = conditional(D, betas)
    return (c + c.T) / (2 * n), betas, tries


def joint(x, perplexity):
    return joint_from_distances(distances(x), perplexity)


def row_entropy(D, i, beta):
    others = np.arange(len(D)) != i
    return entropy(D[i, others] - D[i, others].min(), beta)[0]


# ------------------------------------------------------------------ gradient, KL, the float64 twin of a run
_weights = [None, None]                  # the last layout and its (diff, w): computed once, shared by gradient, KL and the bounds, never written


def weights(y):
    """(y_i - y_j [n x n x 2], w_ij = 1 / (1 + |y_i - y_j|^2) [n x n]) in float64; read-only"""
    y = np.asarray(y, np.float64)
    key = y.tobytes()
    if _weights[0] != key:
        diff = y[:, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (diff * diff).sum(axis=2))
        diff.flags.writeable = w.flags.writeable = False
        _weights[:] = [key, (diff, w)]
    return _weights[1]


def gradient(P, y, exaggeration):
    """g_i = 4 (sum_j e p_ij w_ij (y_i - y_j) - (1 / Z) sum_j w_ij^2 (y_i - y_j)), Z = sum_{i != j} w_ij -> (g, Z)"""
    diff, w = weights(y)
    z = w.sum() - len(w)
    P = np.asarray(P, np.float64)
    return 4.0 * (((exaggeration * P * w)[:, :, None] * diff).sum(axis=1) - ((w * w)[:, :, None] * diff).sum(axis=1) / z), z


def kl(P, y):
    """sum_{p_ij > 0} p_ij log(p_ij Z / w_ij)"""
    _, w = weights(y)
    z = w.sum() - len(w)
    P = np.asarray(P, np.float64)
    on = P > 0
    return float((P[on] * np.log(P[on] * z / w[on])).sum())


def run(P, y0, iterations, eta, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=(0.5, 0.8), min_gain=0.01):
    """the optimisation in float64 (the twin of gr_tsne_run_dev; matrix form) -> final y"""
    P = np.asarray(P, np.float64)
    y = np.asarray(y0, np.float64).copy()
    inc, gains = np.zeros_like(y), np.ones_like(y)
    for t in range(iterations):
        sq = (y * y).sum(axis=1)
        w = 1.0 / (1.0 + np.maximum(sq[:, None] + sq[None, :] - 2.0 * (y @ y.T), 0.0))
        np.fill_diagonal(w, 0.0)
        g = (exaggeration if t < stop_lying_iter else 1.0) * P * w - w * w / w.sum()
        grad = 4.0 * (g.sum(axis=1)[:, None] * y - g @ y)
        gains = np.maximum(np.where(np.sign(grad) == np.sign(inc), gains * 0.8, gains + 0.2), min_gain)
        inc = (momentum[0] if t < mom_switch_iter else momentum[1]) * inc - eta * gains * grad
        y = y + inc
        y = y - y.mean(axis=0)
    return y


def purity(y, labels, k):
    """the share of (point, neighbour) pairs among every point's k nearest neighbours in the map that carry the point's label"""
    y = np.asarray(y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    nearest = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nearest] == labels[:, None]).mean())
