#!/usr/bin/env python3
"""gr_silhouette_dev (csrc/silhouette.hip) at corpus scale: (n, d, k) = (10 000, 100, 20), (100 000, 100, 20), (100 000, 100, 1024) and
(262 144, 32, 20), under both distances.  Nothing is gated: nobody has measured this kernel before, and there is no parent to compare with.
Per shape and metric one call, every kernel under its own pair of events (gr_set_timing 2 / gr_kernel_times): milliseconds per launch, median
[min, max] of 7 calls after one discarded warm-up.  The table is Gaussian noise, the labels uniform over the k clusters.
Next to the pair kernel's time what the contract costs, so the reader sees the distance to the floor:
   fp64 floor     the contract spends 3 separately rounded fp64 operations per pair of rows and column under the euclidean distance (subtract,
                  multiply, add) and 2 under the cosine distance (multiply, add), over all n^2 ordered pairs - the symmetry is not used - at the
                  fp64 vector peak of 78.6 TFLOP/s, which counts a fused multiply-add as two: 39.3 T separately rounded operations per second
                  (the figure tools/bench_mixture.py uses)
Each result is also checked where it was measured: 16 rows' s against a float64 numpy silhouette of those rows (max |difference|).
   python tools/bench_silhouette.py [out.json]      # -> profiles/bench_silhouette.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, FP64_UNFUSED = 7, 78.6e12 / 2
SHAPES = ((10000, 100, 20), (100000, 100, 20), (100000, 100, 1024), (262144, 32, 20))
OPS = {"euclidean": 3, "cosine": 2}
CHECKED_ROWS = 16


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def sampled_difference(np, x, labels, k, metric, rows, values):
    """max |values[i] - s_i| over `rows`, s_i the textbook silhouette of row i in float64 numpy"""
    X = x.astype(np.float64)
    norms = np.sqrt((X * X).sum(axis=1))
    sizes = np.bincount(labels, minlength=k)
    worst = 0.0
    for i in rows:
        if metric == "euclidean":
            dist = np.sqrt(((X - X[i]) ** 2).sum(axis=1))
        else:
            dist = np.maximum(0.0, 1.0 - (X @ X[i]) / (norms * norms[i]))
        dist[i] = 0.0
        sums = np.bincount(labels, weights=dist, minlength=k)
        own = labels[i]
        a = sums[own] / max(sizes[own] - 1, 1)
        means = np.where(sizes > 0, sums / np.maximum(sizes, 1), np.inf)
        means[own] = np.inf
        b = means.min()
        s = (b - a) / max(a, b) if sizes[own] > 1 and np.isfinite(b) and max(a, b) > 0 else 0.0
        worst = max(worst, abs(float(values[i]) - s))
    return worst


def main(path):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    res = {"reps": REPS, "fp64_unfused_ops_per_s": FP64_UNFUSED, "fp64_ops_per_pair_and_column": OPS, "library": os.path.relpath(L.LIB_PATH, ROOT),
           "device": ctx.info(), "rows": []}
    for n, d, k in SHAPES:
        da = DeviceTensor(ctx, (n, d)); ctx.fill_normal(da.ptr, n * d, 7)
        x = da.numpy()
        labels = np.random.default_rng(n + k).integers(0, k, n).astype(np.int32)
        bufs = [ctx.upload(labels)] + [ctx.malloc(b) for b in (8 * n, 8 * k, 4 * k, 8)]
        lab, sv, cmean, sizes, mean = bufs
        try:
            for metric in ("euclidean", "cosine"):
                per = {}
                for rep in range(REPS + 1):
                    ctx.set_timing(2)
                    ctx.silhouette_dev(da.ptr, n, d, lab, k, metric, sv, cmean, sizes, mean); ctx.synchronize()
                    kt = {v["kernel"]: v for v in ctx.kernel_times() if (v["kernel"].startswith("sil_") or v["kernel"] == "wide_group_kernel") and v.get("launches")}
                    ctx.set_timing(0)
                    if rep:                                             # repetition 0 is the warm-up
                        for name, v in kt.items():
                            per.setdefault(name.split("<")[0], []).append(v["total_ms"] / v["launches"])
                        per.setdefault("call", []).append(sum(v["total_ms"] for v in kt.values()))
                values = ctx.download(sv, (n,), np.float64)
                checked = np.random.default_rng(d).choice(n, CHECKED_ROWS, replace=False)
                fp64_ms = float(OPS[metric]) * n * n * d / FP64_UNFUSED * 1e3
                pair = stats(per["sil_pair_kernel"])
                row = {"n": n, "d": d, "k": k, "metric": metric, "fp64_operations": OPS[metric] * n * n * d, "fp64_floor_ms": round(fp64_ms, 4),
                       "kernels_ms_per_launch": {name: stats(v) for name, v in per.items() if name != "call"},
                       "pair_kernel": dict(pair, x_floor=round(pair["ms_median"] / fp64_ms, 2), share_of_floor=round(fp64_ms / pair["ms_median"], 3)),
                       "call_ms": stats(per["call"]), "mean": float(ctx.download(mean, (1,), np.float64)[0]),
                       "checked_rows": CHECKED_ROWS, "max_difference_from_numpy": sampled_difference(np, x, labels, k, metric, checked, values)}
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
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_silhouette.json"))
