"""gr_mst_dev's and gr_hdbscan_host's operations (include/ganrev.h, csrc/mst.hip, csrc/hdbscan.cpp) restated in numpy, and the bounds that say when
two implementations must agree on them.

tree() performs the library's operations where they decide a bit: every pair's distance by silhouette_paths.pair_distances (the chain the
silhouette, the neighbour graph, the eps-graph and the spanning tree share), the core distances as column minSamples - 2 of knn_paths.graph, the
weight max(dist, core_i, core_j) by two comparisons.  The tree itself is found by Kruskal over all pairs sorted by (w, lo, hi): under a strict total
order the minimum spanning tree is unique, so Kruskal must give the tree the library's Boruvka rounds give, edge for edge, and shares no step with
them.  hdbscan() is gr_hdbscan_host's chain: the merges in the order given, the nodes in descending order, one term (lambda - birth) * size per
side that leaves a cluster added in that order from +0.0, the selection in descending cluster number.

Bounds.  u = 2^-53, gamma(m) = m u / (1 - m u), E(v) = knn_paths.distance_bound: how far two implementations' pair distances of value v can lie
apart (valid for any summation order: it covers the library, the restatement, the oracle and scikit-learn alike).
  w                max is 1-Lipschitz and an order statistic is too: a core distance, and so a weight, moves by at most E(its value)
  decided order    the total order of ALL pair distances of a table is decided when every gap between consecutive sorted oracle distances
                   exceeds E(the larger).  Every comparison a correct implementation makes between two weights is a comparison of two pair
                   distances (a weight IS one: the pair's own, or the one behind a core distance), so it comes out as the oracle's, ties as ties -
                   and the tree is the oracle's, edge for edge
  lambda = 1 / w   relative r(w) = E(w) / (w - E(w)) + 2 u (a division each)
  a term           (lambda - birth) * s: |d term| <= s (lambda r(w) + birth r(w_birth)) + 4 u term (a subtraction and a product each)
  stability        m non-negative terms in any order: the terms' bounds added, + 2 gamma(m - 1) stability; second-order terms in 1 + 2^-20
  a comparison     S_children > stability_c is decided when |S - stability_c| exceeds both sides' bounds added
  prob             lambda_row / lambda_max, both of relative error r: r(w_row) + r(w_max) + 2 u, relative; exactly 1 where the two are one number
"""
import math

import numpy as np

from knn_paths import distance_bound, graph
from silhouette_paths import SECOND_ORDER, U64, gamma, pair_distances

import hierarchy_oracle as ho


# ------------------------------------------------------------------ the library's operations
def core_distances(x, min_samples, metric):
    """column minSamples - 2 of the neighbour graph of k = minSamples - 1: the library's bits; None for minSamples 1"""
    return None if min_samples < 2 else np.ascontiguousarray(graph(x, min_samples - 1, metric)["dist"][:, -1])


def weights(dist, core):
    w = np.array(dist, np.float64)
    if core is not None:
        w = np.where(core[:, None] > w, core[:, None], w)               # where core_i > w: core_i
        w = np.where(core[None, :] > w, core[None, :], w)               # where core_j > w: core_j
    return w


def tree(x, min_samples, metric):
    """-> dict(u, v int32, w, core): the library's bits"""
    core = core_distances(x, min_samples, metric)
    u, v, w = ho.kruskal(weights(pair_distances(x, metric), core))
    return dict(u=u.astype(np.int32), v=v.astype(np.int32), w=w, core=core)


def hdbscan(eu, ev, ew, n, min_cluster_size):
    """gr_hdbscan_host's chain -> dict(labels int32, prob, clusters, stability [clusters made], compared [(S, own)])"""
    eu, ev, ew = np.asarray(eu).tolist(), np.asarray(ev).tolist(), np.asarray(ew, np.float64).tolist()
    m = n - 1
    up, node, count = list(range(n)), list(range(n)), [1] * n
    left, right, size = [0] * m, [0] * m, [0] * m

    def find(a):
        while up[a] != a:
            a = up[a]
        return a

    for k in range(m):                                                  # the merges in the order given
        a, b = find(eu[k]), find(ev[k])
        assert a != b
        left[k], right[k], size[k] = node[a], node[b], count[a] + count[b]
        up[b], node[a], count[a] = a, n + k, size[k]
    rows_of = lambda nd: 1 if nd < n else size[nd - n]
    cluster_of = [-1] * m
    cluster_of[m - 1] = 0
    parent, children, birth, stability, lambda_max = [-1], [None], [0.0], [0.0], [0.0]
    row_cluster, row_lambda = [0] * n, [0.0] * n

    def term(c, lam, s):
        t = 0.0 if lam == birth[c] else (lam - birth[c]) * float(s)
        stability[c] = stability[c] + t
        lambda_max[c] = max(lambda_max[c], lam)

    def fall_out(nd, c, lam):
        term(c, lam, rows_of(nd))
        stack = [nd]
        while stack:
            x = stack.pop()
            if x < n:
                row_cluster[x], row_lambda[x] = c, lam
            else:
                stack += [left[x - n], right[x - n]]

    def new_cluster(nd, c, lam):
        parent.append(c); children.append(None); birth.append(lam); stability.append(0.0); lambda_max.append(0.0)
        term(c, lam, rows_of(nd))
        cluster_of[nd - n] = len(parent) - 1
        return len(parent) - 1

    for k in range(m - 1, -1, -1):                                      # descending: every node after its parent
        c = cluster_of[k]
        if c < 0:
            continue
        lam = 1.0 / ew[k] if ew[k] > 0.0 else math.inf
        big_l, big_r = rows_of(left[k]) >= min_cluster_size, rows_of(right[k]) >= min_cluster_size
        if big_l and big_r:
            a = new_cluster(left[k], c, lam)
            b = new_cluster(right[k], c, lam)
            children[c] = (a, b)
        else:
            for nd, big in ((left[k], big_l), (right[k], big_r)):
                if big:
                    cluster_of[nd - n] = c
                else:
                    fall_out(nd, c, lam)
    nc = len(parent)
    own = list(stability)
    selected, compared = [False] + [True] * (nc - 1), []
    for c in range(nc - 1, 0, -1):                                      # descending: every cluster after its children
        if children[c] is None:
            continue
        s = stability[children[c][0]] + stability[children[c][1]]
        compared.append((s, stability[c]))
        if s > stability[c]:
            selected[c], stability[c] = False, s
    owner = [-1] * nc
    for c in range(1, nc):
        owner[c] = owner[parent[c]] if owner[parent[c]] >= 0 else (c if selected[c] else -1)
    labels, prob, number = np.full(n, -1, np.int32), np.zeros(n), {}
    for i in range(n):
        c = owner[row_cluster[i]]
        if c < 0:
            continue
        labels[i] = number.setdefault(c, len(number))
        top = lambda_max[c]
        with np.errstate(invalid="ignore"):
            q = np.float64(row_lambda[i] if row_lambda[i] < top else top) / np.float64(top)
        prob[i] = q if np.isfinite(q) else 1.0
    return dict(labels=labels, prob=prob, clusters=len(number), stability=np.array(own), compared=compared)


# ------------------------------------------------------------------ bounds (two-sided: implementation against implementation)
def order_decided(dist_oracle, d, metric):
    """-> (the number of consecutive sorted pair distances whose order the bounds do not decide, the smallest gap / bound).  Exact ties of the
    oracle (gap 0) count as undecided: the shapes are chosen to have none"""
    n = len(dist_oracle)
    values = np.sort(np.asarray(dist_oracle)[np.triu_indices(n, 1)])
    if len(values) < 2:
        return 0, np.inf
    gaps, room = np.diff(values), distance_bound(values[1:], d, metric)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(room > 0, gaps / room, np.where(gaps > 0, np.inf, 0.0))
    return int((gaps <= room).sum()), float(ratio.min())


def lambda_relative(w, d, metric):
    """r(w): how far two implementations' 1 / w can lie apart, relative; inf where the bound reaches w"""
    w = np.asarray(w, np.float64)
    e = distance_bound(w, d, metric)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w - e > 0, e / (w - e) + 2 * U64, np.inf) * SECOND_ORDER


def stability_bound(cluster, d, metric):
    """cluster: a hierarchy_oracle.Cluster -> how far two implementations' stability of it can lie apart"""
    if not cluster.records:
        return 0.0
    lam = np.array([r[0] for r in cluster.records])
    size = np.array([r[1] for r in cluster.records], np.float64)
    if not np.isfinite(lam).all():
        return np.inf
    rb = float(lambda_relative(1.0 / cluster.birth, d, metric)) if cluster.birth > 0 else 0.0
    terms = (lam - cluster.birth) * size
    each = size * (lam * lambda_relative(1.0 / lam, d, metric) + cluster.birth * rb) + 4 * U64 * terms
    return float((each.sum() + 2 * gamma(len(lam)) * terms.sum()) * SECOND_ORDER)


def subtree_bound(cluster, d, metric):
    """... of the total the selection carries upwards from a cluster: at most every stability below it added, one more sum each"""
    total, count, stack = 0.0, 0, [cluster]
    while stack:
        c = stack.pop()
        total += stability_bound(c, d, metric)
        count += 1
        stack += c.children
    return total * (1 + float(gamma(count + 1)))


def selection_decided(ref, d, metric):
    """ref: hierarchy_oracle.hdbscan's dict -> (the number of excess-of-mass comparisons the bounds do not decide, the smallest |S - own| / bound)"""
    open_, worst = 0, np.inf
    for total, own, c in ref["compared"]:
        room = sum(subtree_bound(k, d, metric) for k in c.children) + stability_bound(c, d, metric) + 4 * U64 * (abs(total) + abs(own))
        gap = abs(total - own)
        if not gap > room:
            open_ += 1
        worst = min(worst, gap / room if room > 0 else np.inf)
    return open_, worst


def prob_bound(ref, d, metric):
    """[n]: how far two implementations' prob can lie apart; 0 where lambda_row reaches lambda_max (the quotient is exactly 1 in every
    implementation once the order of the weights is decided), where either is infinite (1 by rule) and for noise (0 by rule)"""
    row, top = ref["row_lambda"], ref["top_lambda"]
    free = (ref["labels"] >= 0) & np.isfinite(row) & np.isfinite(top) & (row < top)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = lambda_relative(1.0 / np.where(free, row, 1.0), d, metric) + lambda_relative(1.0 / np.where(free, top, 1.0), d, metric) + 2 * U64
    return np.where(free, rel * ref["prob"] * SECOND_ORDER, 0.0)
