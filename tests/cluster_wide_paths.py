"""numpy restatement of gr_cluster_dev's wide route (include/ganrev.h states it; csrc/kmeans.hip): which route a call takes, the stable grouping of
512-row blocks by label, and the arithmetic contract - sequential fp32 dot products with separately rounded multiply and add, first maximum over
ascending j, fp64 member sums per 512-row block in row order and over the blocks in block order, one rounding to fp32, one fp32 division."""
import numpy as np

WIDE_MIN_K = 33              # kmeans.hip g_cluster_wide_min_k, gr_set_tuning "cluster_wide_min_k"
NARROW_MAX_K = 32            # kmeans.hip KM_KMAX: the registers of kmeans_assign_kernel
NARROW_LDS_BYTES = 60 * 1024  # launch_kmeans: k x d doubles of kmeans_accumulate_kernel
MAX_K, MAX_D, MAX_M = 4096, 256, 128
ROWS_PER_BLOCK = 512         # kernels.h ROWS_PER_BLOCK
CENTROID_TILE = 128          # kmeans.hip KW_KT: centroids staged per tile of kmeans_assign_wide_kernel
CENTROIDS_PER_THREAD = 16    # a half-wave's share of the tile
ROWS_PER_WORKGROUP = 128     # kmeans.hip KW_TR


def route(k, d, min_k=WIDE_MIN_K):
    """'narrow': the launches of gr_kmeans_dev, gr_cosine_assign_dev, gr_cluster_members_dev; 'wide': the wide kernels"""
    if not (1 <= k <= MAX_K and 1 <= d <= MAX_D):
        return "unsupported"
    return "wide" if k >= min_k or k > NARROW_MAX_K or k * d * 8 > NARROW_LDS_BYTES else "narrow"


def segment_slots(k):
    return min(k, ROWS_PER_BLOCK)


def workspace_ints_and_doubles(n, d, k):
    """the wide route's scratch as the header states it: (ints, doubles)"""
    B = -(-n // ROWS_PER_BLOCK)
    S = B * segment_slots(k)
    return 2 * S + 2 * B + ROWS_PER_BLOCK * B + n, S * d


def group_block(labels, k):
    """one block's labels -> (order: positions in (label, row) order; seg_label ascending; seg_start: first entry of each segment in `order`)"""
    labels = np.asarray(labels)
    valid = np.nonzero((labels >= 0) & (labels < k))[0]
    keys = labels[valid].astype(np.int64) * ROWS_PER_BLOCK + valid          # distinct: the sort the kernel does
    order = valid[np.argsort(keys)]
    lab = labels[order]
    heads = np.nonzero(np.r_[True, lab[1:] != lab[:-1]])[0] if len(order) else np.zeros(0, np.int64)
    return order, lab[heads], heads


def group(labels, k):
    """all blocks: the grouped row index (rows of a block stay in that block's stretch) and per block (seg_label, seg_start, rows in the block)"""
    labels = np.asarray(labels)
    order, blocks = [], []
    for r0 in range(0, len(labels), ROWS_PER_BLOCK):
        o, sl, ss = group_block(labels[r0:r0 + ROWS_PER_BLOCK], k)
        order.append(o + r0)
        blocks.append((sl, ss, len(o)))
    return order, blocks


def c2_of(cent):
    """kmeans_c2_kernel / kmeans_update_kernel: fp32 squares, sequential fp64 sum in column order, one rounding, times 0.5f"""
    p = (cent * cent).astype(np.float32)
    s = np.zeros(len(cent), np.float64)
    for t in range(cent.shape[1]):
        s = s + p[:, t].astype(np.float64)
    return s.astype(np.float32) * np.float32(0.5)


def scores(x, cent, c2):
    """[n, k] fp32: per pair one chain in column order, s = s + c[j][t] * x[i][t] (both roundings), then s - c2[j]"""
    s = np.zeros((len(x), len(cent)), np.float32)
    for t in range(x.shape[1]):
        s = s + cent[None, :, t] * x[:, None, t]
    return s - c2[None, :]


def first_maximum(v):
    """labels of the sequential scan `j == 0 or v[j] > best`: the largest value, the lowest index among equals; a NaN score 0 keeps label 0, a NaN
    elsewhere never wins"""
    w = np.where(np.isnan(v), -np.inf, v)
    lab = np.argmax(w, axis=1)
    lab[np.isnan(v[:, 0])] = 0
    return lab.astype(np.int32)


def member_sums(x, labels, k):
    """-> (totals fp64 [k, d], counts int [k]): per 512-row block a cluster's rows in row order from +0.0, the blocks' partials in block order"""
    d = x.shape[1]
    total = np.zeros((k, d), np.float64)
    counts = np.zeros(k, np.int64)
    for r0 in range(0, len(x), ROWS_PER_BLOCK):
        lab = labels[r0:r0 + ROWS_PER_BLOCK]
        part = np.zeros((k, d), np.float64)
        np.add.at(part, lab, x[r0:r0 + ROWS_PER_BLOCK].astype(np.float64))        # unbuffered: one row after the other
        here = np.unique(lab)
        total[here] = total[here] + part[here]                                      # a block without a member adds nothing
        counts += np.bincount(lab, minlength=k)
    return total, counts


def kmeans(x, k, niter, c0):
    """unsup.kmeans as gr_cluster_dev computes it -> (centroids fp32 [k, d], totalcounts fp32 [k], labels int32 [n] of the last iteration)"""
    x = np.ascontiguousarray(x, np.float32)
    cent = np.array(c0, np.float32)
    tot = np.zeros(k, np.float32)
    labels = np.zeros(len(x), np.int32)
    c2 = c2_of(cent)
    for _ in range(niter):
        labels = first_maximum(scores(x, cent, c2))
        total, counts = member_sums(x, labels, k)
        got = counts > 0                                                             # a cluster without a row keeps its centroid and its c2
        cent[got] = total[got].astype(np.float32) / counts[got].astype(np.float32)[:, None]
        c2 = c2_of(cent)
        tot = tot + counts.astype(np.float32)
    return cent, tot, labels


def case(N, d, k):
    """the data of the issue's cases: rng(N + k), standard normal rows with the first third shifted, normalised normal centroids"""
    rng = np.random.default_rng(N + k)
    x = rng.standard_normal((N, d)).astype(np.float32)
    x[: N // 3] += np.float32(1.5)
    c0 = rng.standard_normal((k, d)).astype(np.float32)
    c0 /= np.linalg.norm(c0, axis=1, keepdims=True)
    return x, c0.astype(np.float32)


# (N, d, k, niter): above 32 clusters; the first four also run against the oracle without a GPU
HOST_CASES = [(1300, 33, 33, 3), (5000, 33, 257, 3), (5000, 100, 1024, 2), (20000, 32, 64, 4)]
GPU_ONLY_CASES = [(700, 256, 64, 2), (5000, 8, 4096, 1), (70001, 8, 257, 1)]
