#!/usr/bin/env python3
"""gr_knn_dev (csrc/knn.hip) at corpus scale: (n, d, k) = (10 000, 100, 20), (100 000, 100, 20) and (100 000, 100, 128), under both distances, and
beside each the yardstick: gr_silhouette_dev's pair kernel on the same table with 20 clusters - the same pair arithmetic, with 64 ordered adds
per row and tile where the graph has 64 compares and its insertions.  Both are timed in one process, in alternating calls (one graph, one
silhouette, seven times after one discarded round), every kernel under its own pair of events (gr_set_timing 2 / gr_kernel_times): milliseconds
per launch, median [min, max].  The ratio knn_pair_kernel / sil_pair_kernel is what DESIGN.md holds against 1.16 at k = 20; at k = 128 it is
reported.  The table is Gaussian noise, in random order: the lists then cost about k ln(n / k) insertions per row.
Each graph is also checked where it was measured: 16 rows' lists against a float64 numpy sort of those rows' distances.
   python tools/bench_knn.py [out.json]      # -> profiles/bench_knn.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, CLUSTERS, CHECKED_ROWS = 7, 20, 16
SHAPES = ((10000, 100, 20), (100000, 100, 20), (100000, 100, 128))


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def sampled_check(np, x, metric, rows, idx, dist):
    """(rows whose list differs from float64 numpy's, max |dist - numpy's|) over `rows`"""
    X = x.astype(np.float64)
    norms = np.sqrt((X * X).sum(axis=1))
    wrong, worst = 0, 0.0
    for i in rows:
        if metric == "euclidean":
            dd = np.sqrt(((X - X[i]) ** 2).sum(axis=1))
        else:
            dd = np.maximum(0.0, 1.0 - (X @ X[i]) / (norms * norms[i]))
        dd[i] = np.inf
        order = np.lexsort((np.arange(len(X)), dd))[:idx.shape[1]]
        wrong += int(not np.array_equal(order, idx[i]))
        worst = max(worst, float(np.abs(dd[order] - dist[i]).max()))
    return wrong, worst


def kernel_ms(ctx, prefix):
    return {v["kernel"]: v["total_ms"] / v["launches"] for v in ctx.kernel_times() if v["kernel"].startswith(prefix) and v.get("launches")}


def main(path):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    res = {"reps": REPS, "silhouette_clusters": CLUSTERS, "library": os.path.relpath(L.LIB_PATH, ROOT), "device": ctx.info(), "rows": []}
    for n, d, k in SHAPES:
        da = DeviceTensor(ctx, (n, d)); ctx.fill_normal(da.ptr, n * d, 7)
        x = da.numpy()
        labels = np.random.default_rng(n + CLUSTERS).integers(0, CLUSTERS, n).astype(np.int32)
        bufs = [ctx.upload(labels)] + [ctx.malloc(b) for b in (8 * n, 8 * CLUSTERS, 4 * CLUSTERS, 8, 4 * n * k, 8 * n * k)]
        lab, sv, cmean, sizes, mean, idx_dev, dist_dev = bufs
        try:
            for metric in ("euclidean", "cosine"):
                knn, sil = [], []
                for rep in range(REPS + 1):                             # round 0 is the warm-up
                    ctx.set_timing(2)
                    ctx.knn_dev(da.ptr, n, d, k, metric, idx_dev, dist_dev); ctx.synchronize()
                    a = kernel_ms(ctx, "knn_pair_kernel")
                    ctx.set_timing(0); ctx.set_timing(2)
                    ctx.silhouette_dev(da.ptr, n, d, lab, CLUSTERS, metric, sv, cmean, sizes, mean); ctx.synchronize()
                    b = kernel_ms(ctx, "sil_pair_kernel")
                    ctx.set_timing(0)
                    if rep:
                        knn.append(sum(a.values())); sil.append(sum(b.values()))
                idx, dist = ctx.download(idx_dev, (n, k), np.int32), ctx.download(dist_dev, (n, k), np.float64)
                checked = np.random.default_rng(d).choice(n, CHECKED_ROWS, replace=False)
                wrong, worst = sampled_check(np, x, metric, checked, idx, dist)
                ks, ss = stats(knn), stats(sil)
                row = {"n": n, "d": d, "k": k, "metric": metric, "knn_pair_kernel": ks, "sil_pair_kernel": ss,
                       "ratio_of_medians": round(ks["ms_median"] / ss["ms_median"], 3), "ratio_of_minima": round(ks["ms_min"] / ss["ms_min"], 3),
                       "checked_rows": CHECKED_ROWS, "rows_whose_list_differs_from_numpy": wrong, "max_distance_difference_from_numpy": worst}
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        finally:
            for b in bufs:
                ctx.free(b)
            da.free()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_knn.json"))
