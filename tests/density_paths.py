"""gr_eps_graph_dev's and gr_dbscan_dev's operations (include/ganrev.h, csrc/density.hip) restated in numpy, and what decides whether two
implementations must agree on them.

graph() performs the library's operations in the library's order: every pair's distance by silhouette_paths.pair_distances (the chain the
silhouette, the neighbour graph and the eps-graph share), one comparison dist <= eps per pair, the diagonal set, the bits packed 64 to a word
(bit j % 64 of word j / 64), the popcounts.  labels() is the rule as the header states it - core rows, the connected components of the core rows,
numbered by their smallest core row, border rows to the lowest number among their core neighbours, -1 for the rest - by a union-find, which shares
nothing with the library's hook-and-compress rounds nor with the oracle's breadth-first expansion.

Decided pairs.  A bit is a comparison of a distance with eps, so two correct implementations can differ only on a pair whose distance lies within
their combined error of eps: |dist - eps| <= E(max(dist, eps)), E = knn_paths.distance_bound (twice the one-sided error of the fp64 chain, valid
for any summation order, so it covers the library, the restatement and the oracle alike).  undecided() counts those pairs on the oracle's distances.
The tests choose eps so that there are none (eps_for: the middle of the widest gap between consecutive distinct pair distances near the wanted
quantile): words, counts, core flags and labels must then equal the oracle's exactly.
"""
import numpy as np

from knn_paths import distance_bound
from silhouette_paths import pair_distances

import density_oracle as do


# ------------------------------------------------------------------ the library's operations
def pack(adj):
    """[n x n] bool -> [n x ceil(n / 64)] uint64: bit j % 64 of word j / 64; the bits at and past n are 0"""
    adj = np.asarray(adj, bool)
    n = adj.shape[1]
    padded = np.zeros((len(adj), (n + 63) // 64 * 64), np.uint8)
    padded[:, :n] = adj
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8")


def unpack(words, n):
    """[rows x ceil(n / 64)] uint64 -> [rows x n] bool, and the padding bits [rows x (64 ceil(n / 64) - n)]"""
    bits = np.unpackbits(np.ascontiguousarray(words).astype("<u8").view(np.uint8), axis=1, bitorder="little").astype(bool)
    return bits[:, :n], bits[:, n:]


def graph(x, eps, metric):
    """-> dict(words [n x ceil(n / 64)] uint64, count [n] int32, adj [n x n] bool): the library's bits"""
    adj = pair_distances(x, metric) <= eps
    np.fill_diagonal(adj, True)                                         # a row is in its own neighbourhood
    return dict(words=pack(adj), count=adj.sum(axis=1).astype(np.int32), adj=adj)


def labels(adj, count, min_pts):
    """the rule of include/ganrev.h -> (labels [n] int32, core [n] bool, the number of clusters)"""
    adj, count = np.asarray(adj, bool), np.asarray(count)
    n = len(count)
    core = count >= min_pts
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    among = adj & core[None, :] & core[:, None]
    for i, j in np.argwhere(np.triu(among, 1)).tolist():                # the components of the core rows ...
        a, b = find(i), find(j)
        if a != b:
            root[max(a, b)] = min(a, b)                                 # ... each under its smallest core row
    roots = np.array([find(i) if core[i] else -1 for i in range(n)])
    number = np.full(n, -1, np.int64)
    first = np.unique(roots[core])                                      # ascending: clusters are numbered by their smallest core row
    number[first] = np.arange(len(first))
    out = np.full(n, -1, np.int32)
    out[core] = number[roots[core]]
    for i in np.nonzero(~core)[0]:
        near = np.nonzero(adj[i] & core)[0]
        if len(near):
            out[i] = out[near].min()                                    # a border row: the lowest cluster number among its core neighbours
    return out, core, len(first)


# ------------------------------------------------------------------ what decides a bit
def undecided(dist_oracle, eps, d, metric):
    """-> (the number of pairs i != j whose bit the bounds do not decide, the smallest |dist - eps| / bound over those pairs; inf without a pair)"""
    dist = np.asarray(dist_oracle, np.float64)
    off = ~np.eye(len(dist), dtype=bool)
    gap = np.abs(dist - eps)[off]
    room = distance_bound(np.maximum(dist, eps), d, metric)[off]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(room > 0, gap / room, np.where(gap > 0, np.inf, 0.0))
    return int((gap <= room).sum()), float(ratio.min()) if ratio.size else np.inf


def eps_for(x, min_pts, q, metric, dist_oracle=None, window=200):
    """An eps near the k-distance rule's that no pair distance comes close to: the target is the q-quantile of the rows' distances to their
    (min_pts - 1)-th nearest other row (the nearest for min_pts < 2, and never past the last); among the `window` distinct oracle pair distances
    around the target, the midpoint of the widest gap.  Two rows have one distance: half of it for q < 0.5, twice it otherwise."""
    dist = do.distances(x, metric) if dist_oracle is None else np.asarray(dist_oracle)
    n = len(dist)
    if n == 2:
        return float(dist[0, 1]) * (0.5 if q < 0.5 else 2.0)
    target = np.quantile(do.kdistances(dist, min(max(min_pts - 1, 1), n - 1)), q)
    values = np.unique(dist[np.triu_indices(n, 1)])
    at = int(np.searchsorted(values, target))
    lo = max(0, min(at - window // 2, len(values) - window))
    near = values[lo:lo + window]
    if len(near) < 2:                                                   # one distinct distance: anywhere off it
        return float(near[0]) * 0.5 if near[0] > 0 else 1.0
    widest = int(np.argmax(np.diff(near)))
    return float((near[widest] + near[widest + 1]) / 2)
