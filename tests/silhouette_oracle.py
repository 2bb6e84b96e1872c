"""float64 numpy reference of gr_silhouette_dev (include/ganrev.h): the silhouette coefficient in its textbook form - a row's distances to all rows,
summed per cluster by numpy - with the rules of the library: a label outside [0, k) is no cluster, a singleton scores 0, a row without another
cluster to compare with scores 0, a zero row has cosine 0 to every row.  No grouping, no tiles, no chain order.  And the inputs of the tests."""
import numpy as np

METRICS = ("euclidean", "cosine")


def distances_from(X, norms, i, metric):
    """the distances of row i to every row [n]; its own entry is 0"""
    if metric == "euclidean":
        dist = np.sqrt(((X - X[i]) ** 2).sum(axis=1))
    else:
        den = norms * norms[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(den > 0, (X @ X[i]) / den, 0.0)
        dist = np.maximum(0.0, 1.0 - c)
    dist[i] = 0.0
    return dist


def silhouette(x, labels, k, metric):
    """-> dict(values, a, b [n], nearest [n], cluster_mean [k], sizes [k], mean; gap [n]: the second smallest other-cluster mean minus the smallest,
    inf without a second - how far `nearest` is from flipping)"""
    assert metric in METRICS
    X, labels = np.asarray(x, np.float64), np.asarray(labels, np.int64)
    n = len(X)
    valid = (labels >= 0) & (labels < k)
    lab = np.where(valid, labels, 0)
    sizes = np.bincount(lab[valid], minlength=k)
    norms = np.sqrt((X * X).sum(axis=1))
    values, a, b, gap = np.zeros(n), np.zeros(n), np.zeros(n), np.full(n, np.inf)
    nearest = np.full(n, -1, np.int64)
    for i in np.nonzero(valid)[0]:
        dist = distances_from(X, norms, i, metric)
        sums = np.bincount(lab[valid], weights=dist[valid], minlength=k)
        own = labels[i]
        if sizes[own] > 1:
            a[i] = sums[own] / (sizes[own] - 1)
        other = sizes > 0
        other[own] = False
        if not other.any():
            continue
        means = np.where(other, sums / np.maximum(sizes, 1), np.inf)
        nearest[i] = int(means.argmin())                                # numpy's argmin: the first minimum
        b[i] = means[nearest[i]]
        rest = np.delete(means, nearest[i])
        gap[i] = rest.min() - b[i] if len(rest) else np.inf
        top = max(a[i], b[i])
        if sizes[own] > 1 and top > 0:
            values[i] = (b[i] - a[i]) / top
    cluster_mean = np.array([values[valid & (labels == c)].mean() if sizes[c] else 0.0 for c in range(k)])
    return dict(values=values, a=a, b=b, nearest=nearest, cluster_mean=cluster_mean, sizes=sizes, mean=float(values.mean()), gap=gap)


# ------------------------------------------------------------------ inputs
def blobs(n, d, groups, seed, spread=3.0):
    """n float32 rows around `groups` Gaussian centres `spread` apart per column, unit spread around each -> (x [n x d], the group of each row);
    distances between rows are of order sqrt(d), cosine distances of order 1"""
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((groups, d))
    group = rng.integers(0, groups, n)
    return (centres[group] + rng.standard_normal((n, d))).astype(np.float32), group


def labels_of_sizes(sizes, seed):
    """a labelling with exactly sizes[c] rows of cluster c, the rows in shuffled order"""
    labels = np.repeat(np.arange(len(sizes)), sizes)
    np.random.default_rng(seed).shuffle(labels)
    return labels.astype(np.int32)
