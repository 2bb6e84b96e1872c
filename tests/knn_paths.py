"""gr_knn_dev's, gr_lof_dev's and gr_knn_overlap_dev's operation chains (include/ganrev.h, csrc/knn.hip) restated in numpy, and the error bounds that
follow from them.

graph() performs the library's operations in the library's order: every pair's distance by silhouette_paths.pair_distances (the chain the two calls
share), then the selection - the rows j != i visited in ascending order, one entering the list only where its distance is below the list's k-th,
behind its equals: the first k of a stable sort by distance.  lof() adds the k reach values and the k neighbour densities in list order from +0.0,
every operation rounded on its own; overlap() takes the mean of count / k by chain.hip's 512-row chain (silhouette_paths.chain_mean).

Bounds.  u = 2^-53, gamma(m) = m u / (1 - m u) (silhouette_paths).  As there, every sum below is a sum of non-negative terms, so a bound holds for ANY
summation order: it covers the library's chain, the restatement and the oracle's numpy means alike, and a comparison of two such implementations is
within twice the one-sided figure; the functions return the doubled figure.  E(v) = 2 (e_abs + e_rel v) (1 + 2^-20) is that figure for a pair
distance of (oracle) value v, (e_abs, e_rel) = silhouette_paths.distance_error(d, metric); it grows with v.
  dist[i][p]       the p-th smallest of row i's n - 1 distances.  An order statistic is 1-Lipschitz in the sup norm: if every distance moves by at
                   most E(its value), the p-th smallest moves by at most E(the p-th smallest) - whatever the neighbour order.  E(dist[i][p])
  decided rows     a row's list is decided when every gap between consecutive oracle distances among its first k + 1 neighbours (k where the table
                   has no more) exceeds E(the larger of the two): no two of them can change places in either implementation
  reach            max is 1-Lipschitz too: max(E(kdist_j), E(dist[i][p])) = E(reach), E being monotone
  m_i              k non-negative terms and a division: gamma(k + 2) relative per implementation.  Dm_i = mean_p E(reach_ip) + 2 gamma(k + 2) m_i
  lrd_i            1 / (m_i + 1e-10): the addition and the reciprocal round once each per implementation.  Relative:
                   r_i = Dm_i / (m_i + 1e-10 - Dm_i) + 4 u
  lof_i            the numerator is a mean of positive terms of relative error <= max_p r_(j_p), + 2 gamma(k + 2) for the sum and the division;
                   the quotient adds r_i and 2 u: lof_i ((max_p r_j + 2 gamma(k + 2) + r_i + 2 u) / (1 - r_i)), second-order terms in 1 + 2^-20
  overlap          the counts are integers: exact where both graphs' rows are decided.  mean: n terms count / k <= 1, one rounding each, a sum and a
                   division: 2 gamma(n + 3) absolute
"""
import numpy as np

from silhouette_paths import SECOND_ORDER, U64, chain_mean, distance_error, gamma, pair_distances

LRD_EPSILON = 1e-10         # include/ganrev.h: lrd = 1 / (m + 1e-10)


# ------------------------------------------------------------------ the library's chains
def graph(x, k, metric):
    """-> dict(idx [n x k] int32, dist [n x k]): the library's bits"""
    dist = pair_distances(x, metric)
    np.fill_diagonal(dist, np.inf)                                      # a row is not its own neighbour
    idx = np.argsort(dist, axis=1, kind="stable")[:, :k]                # ascending j, strict <: behind its equals
    return dict(idx=idx.astype(np.int32), dist=np.take_along_axis(dist, idx, axis=1))


def lof(idx, dist):
    """-> (lof, lrd): the library's bits"""
    idx, dist = np.asarray(idx, np.int64), np.asarray(dist, np.float64)
    n, k = idx.shape
    kdist = dist[:, k - 1]
    m = np.zeros(n)
    for p in range(k):                                                  # list order, from +0.0
        m = m + np.maximum(kdist[idx[:, p]], dist[:, p])
    m = m / float(k)
    lrd = 1.0 / (m + LRD_EPSILON)
    s = np.zeros(n)
    for p in range(k):
        s = s + lrd[idx[:, p]]
    s = s / float(k)
    return s / lrd, lrd


def overlap(idx_a, idx_b):
    """-> (count [n] int32, mean): the library's bits"""
    idx_a, idx_b = np.asarray(idx_a), np.asarray(idx_b)
    k = idx_a.shape[1]
    count = (idx_a[:, :, None] == idx_b[:, None, :]).any(axis=2).sum(axis=1).astype(np.int32)
    return count, chain_mean(count.astype(np.float64) / float(k))


# ------------------------------------------------------------------ bounds (two-sided: implementation against implementation)
def distance_bound(values, d, metric):
    """E(v): how far two implementations' pair distances of oracle value v can lie apart"""
    e_abs, e_rel = distance_error(d, metric)
    return 2.0 * (e_abs + e_rel * np.asarray(values, np.float64)) * SECOND_ORDER


def decided(ref, d, metric):
    """ref: knn_oracle.knn's dict -> (decided [n] bool, the smallest gap / bound over all rows and places; inf without a gap)"""
    ahead = ref["ahead"]
    if ahead.shape[1] < 2:
        return np.ones(len(ahead), bool), np.inf
    gaps, room = np.diff(ahead, axis=1), distance_bound(ahead[:, 1:], d, metric)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(room > 0, gaps / room, np.where(gaps > 0, np.inf, 0.0))
    return (gaps > room).all(axis=1), float(ratio.min())


def lof_bounds(ref, ref_lof, ref_lrd, d, metric):
    """ref: knn_oracle.knn's dict, ref_lof / ref_lrd: knn_oracle.lof of it -> dict(dist [n x k], lrd [n], lof [n], lof_relative [n])"""
    idx, dist = ref["idx"], ref["dist"]
    k = idx.shape[1]
    reach = np.maximum(dist[:, -1][idx], dist)
    m = reach.mean(axis=1)
    dm = distance_bound(reach, d, metric).mean(axis=1) + 2 * gamma(k + 2) * m
    room = m + LRD_EPSILON - dm
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(room > 0, dm / room + 4 * U64, np.inf) * SECOND_ORDER
        rel = (r[idx].max(axis=1) + 2 * gamma(k + 2) + r + 2 * U64) / np.where(r < 1, 1 - r, 0.0) * SECOND_ORDER
    rel = np.where(np.isfinite(rel), rel, np.inf)
    return dict(dist=distance_bound(dist, d, metric), lrd=r * ref_lrd, lof=rel * ref_lof, lof_relative=rel)


def overlap_mean_bound(n):
    return float(2 * gamma(n + 3))
