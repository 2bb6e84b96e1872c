"""gr_silhouette_dev's operation chains (include/ganrev.h, csrc/silhouette.hip) restated in numpy, and the error bounds that follow from them.

chain() performs the library's operations in the library's order: every pair's distance one fp64 chain in column order with the multiply and the
add rounded separately, a cluster's members added in ascending row order from +0.0 (the row itself as +0.0, which leaves the bits), the first
minimum over ascending clusters, the members' s in row order, the mean by the 512-row chain of chain.hip.

Bounds.  u = 2^-53, gamma(m) = m u / (1 - m u).  Every bound below holds for ANY summation order, because every sum that enters a, b is a sum of
non-negative terms (distances) and |s| <= 1: it covers the library's chain, the restatement and the oracle's numpy sums alike.  A comparison of two
such implementations is within twice the one-sided bound; the functions return that doubled figure.
  euclidean distance   t = fl(x_i - x_j) carries u, t t two more and its own rounding: 3 u per term; d - 1 adds of non-negative terms: D within
                       gamma(d + 2) relative; the root halves that and adds u: dist within gamma(d + 4) relative (generous by a factor of 2)
  cosine distance      p within gamma(d + 1) sum |x_it x_jt| <= gamma(d + 1) q_i q_j (Cauchy-Schwarz); q within gamma(d + 3) relative; q_i q_j
                       within gamma(2 d + 8); c = p / (q_i q_j), |c| <= 1, within gamma(3 d + 12) absolute; 1 - c adds 2 u; clamping at 0 moves
                       towards the true value, which is >= 0: dist within gamma(3 d + 16) ABSOLUTE
  a mean of m dists    the sum adds gamma(m - 1) relative, the division u: E_abs + (E_rel + gamma(m + 2)) mean, second-order terms in a factor
                       1 + 2^-20
  a                    that with m = size_own - 1;  b: the minimum of such means - (1 - e) f - E <= f^ <= (1 + e) f + E for every cluster moves the
                       minimum by no more - with m = the largest other cluster
  s = (b - a) / max    |ds/da|, |ds/db| <= 1 / max(a, b): (Da + Db) / (max(a, b) - Da - Db) + 3 u (the subtraction, the division, |s| <= 1); 0 where
                       the rules give s = 0
  cluster_mean, mean   the mean of the members' (all rows') bounds on s, + gamma(size + 1) (gamma(n + 1)) for the sum and the division
"""
import numpy as np

U64 = 2.0 ** -53
ROWS_PER_BLOCK = 512        # kernels.h
SECOND_ORDER = 1.0 + 2.0 ** -20


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U64 / (1.0 - m * U64)


# ------------------------------------------------------------------ the library's chains
def ordered_sum(values):
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def chain_mean(values):
    """chain.hip: per block of 512 rows in row order from +0.0, the partials in block order from +0.0, one division"""
    values = np.asarray(values, np.float64)
    parts = [ordered_sum(values[lo:lo + ROWS_PER_BLOCK]) for lo in range(0, len(values), ROWS_PER_BLOCK)]
    return ordered_sum(parts) / float(len(values))


def pair_distances(x, metric):
    """[n x n] by the library's chain; the diagonal is +0.0 (a row is not its own neighbour)"""
    X = np.asarray(x, np.float32).astype(np.float64)
    n, d = X.shape
    acc = np.zeros((n, n))
    if metric == "euclidean":
        for t in range(d):
            df = X[:, t, None] - X[None, :, t]
            acc = acc + df * df
        dist = np.sqrt(acc)
    else:
        qq = np.zeros(n)
        for t in range(d):
            acc = acc + X[:, t, None] * X[None, :, t]
            qq = qq + X[:, t] * X[:, t]
        q = np.sqrt(qq)
        den = q[:, None] * q[None, :]
        zero = (q[:, None] == 0.0) | (q[None, :] == 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(zero, 0.0, acc / den)
        e = 1.0 - c
        dist = np.where(e > 0.0, e, 0.0)
    np.fill_diagonal(dist, 0.0)
    return dist


def chain(x, labels, k, metric):
    """-> dict(values, a, b, nearest, cluster_mean, sizes, mean): the library's bits"""
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    valid = (labels >= 0) & (labels < k)
    dist = pair_distances(x, metric)
    sizes = np.bincount(labels[valid], minlength=k)
    occupied = np.nonzero(sizes)[0]
    sums = np.zeros((n, len(occupied)))
    for col, c in enumerate(occupied):
        run = np.zeros(n)
        for j in np.nonzero(valid & (labels == c))[0]:                  # ascending rows
            run = run + dist[:, j]
        sums[:, col] = run
    values, a, b = np.zeros(n), np.zeros(n), np.zeros(n)
    nearest = np.full(n, -1, np.int64)
    col_of = {int(c): col for col, c in enumerate(occupied)}
    for i in np.nonzero(valid)[0]:
        own = int(labels[i])
        if sizes[own] > 1:
            a[i] = sums[i, col_of[own]] / float(sizes[own] - 1)
        best = None
        for col, c in enumerate(occupied):                              # ascending clusters, the first minimum
            if c == own:
                continue
            mc = sums[i, col] / float(sizes[c])
            if best is None or mc < best:
                best, nearest[i] = mc, c
        if best is None:
            continue
        b[i] = best
        top = a[i] if a[i] > b[i] else b[i]
        if sizes[own] > 1 and top != 0.0:
            values[i] = (b[i] - a[i]) / top
    cluster_mean = np.array([ordered_sum(values[valid & (labels == c)]) / float(sizes[c]) if sizes[c] else 0.0 for c in range(k)])
    return dict(values=values, a=a, b=b, nearest=nearest, cluster_mean=cluster_mean, sizes=sizes, mean=chain_mean(values))


# ------------------------------------------------------------------ bounds (two-sided: implementation against implementation)
def distance_error(d, metric):
    """(absolute, relative) one-sided error of a pair distance"""
    return (0.0, float(gamma(d + 4))) if metric == "euclidean" else (float(gamma(3 * d + 16)), 0.0)


def bounds(ref, labels, k, d, metric):
    """ref: the oracle's dict -> dict(a, b, values [n], cluster_mean [k], mean, undecided [n] bool: rows whose `nearest` the bounds do not decide)"""
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    valid = (labels >= 0) & (labels < k)
    sizes = np.asarray(ref["sizes"], np.int64)
    e_abs, e_rel = distance_error(d, metric)
    own_size = np.where(valid, sizes[np.where(valid, labels, 0)], 0)
    # the largest cluster other than the row's own
    order = np.argsort(-sizes, kind="stable")
    largest, second = int(order[0]), int(order[1]) if k > 1 else int(order[0])
    other_size = np.where(np.where(valid, labels, -1) == largest, sizes[second] if k > 1 else 0, sizes[largest])
    a1 = (e_abs + (e_rel + gamma(np.maximum(own_size - 1, 1) + 2)) * ref["a"]) * SECOND_ORDER
    b1 = (e_abs + (e_rel + gamma(other_size + 2)) * ref["b"]) * SECOND_ORDER
    ruled = ~valid | (own_size <= 1) | (ref["nearest"] < 0)             # s = 0 by rule
    a1 = np.where(~valid | (own_size <= 1), 0.0, a1)
    b1 = np.where(~valid | (ref["nearest"] < 0), 0.0, b1)
    top = np.maximum(ref["a"], ref["b"])
    room = top - a1 - b1
    with np.errstate(divide="ignore", invalid="ignore"):
        s1 = np.where(room > 0, (a1 + b1) / room + 3 * U64, np.where(a1 + b1 == 0, 0.0, np.inf))
    s1 = np.where(ruled, 0.0, s1)
    member = [valid & (labels == c) for c in range(k)]
    cm1 = np.array([s1[member[c]].mean() + gamma(sizes[c] + 1) if sizes[c] else 0.0 for c in range(k)])
    mean1 = float(s1.mean() + gamma(n + 1))
    # `nearest` can differ between two implementations only where the two smallest means, each moved by its error in both, can cross
    gap = np.where(np.isfinite(ref["gap"]), ref["gap"], 0.0)
    undecided = valid & (ref["nearest"] >= 0) & np.isfinite(ref["gap"]) & (gap <= 4 * (e_abs + (e_rel + gamma(sizes.max() + 2)) * (ref["b"] + gap)) * SECOND_ORDER)
    return dict(a=2 * a1, b=2 * b1, values=2 * s1, cluster_mean=2 * cm1, mean=2 * mean1, undecided=undecided, values_one_sided=s1)
