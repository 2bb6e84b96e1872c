#!/usr/bin/env python3
"""gr_mst_dev (csrc/mst.hip) and gr_hdbscan_host (csrc/hdbscan.cpp) at corpus scale: bench_knn.py's shapes (n, d) = (10 000, 100) and
(100 000, 100), under both distances, minSamples 1 (plain single linkage) and 10 (core distances read in place from column 8 of a gr_knn_dev
graph of 9 neighbours, built once outside the timing).  Beside the tree's pair kernel stands the yardstick: gr_silhouette_dev's pair kernel on
the same table with 20 clusters - the same pair arithmetic, with 64 ordered adds per row and tile where the tree has one compare per pair and
four shuffles per row at the end.  Both are timed in one process, in alternating calls (one tree, one silhouette, seven times after one discarded
round), every kernel under its own pair of events (gr_set_timing 2 / gr_kernel_times): mst_pair_kernel in milliseconds per Boruvka round (its
total over its launches), the component pass (memset, two atomicMin kernels, hook, compress) and the final ranking as totals per call, the
rounds taken, and the wall time of the call with its stream waits; median [min, max].  gr_hdbscan_host is timed on the finished tree
(minClusterSize 25).  The table is Gaussian noise.
Each tree is also checked where it was measured: for 16 rows, float64 numpy's smallest weight over all pairs of the row - an edge every minimum
spanning tree holds - must be among the row's tree edges (where the runner-up is more than 1e-9 away), and every weight of the row's tree edges
must agree with float64 numpy within 1e-9.
   python tools/bench_hierarchy.py [out.json]      # -> profiles/bench_hierarchy.json"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, CLUSTERS, CHECKED_ROWS, MIN_CLUSTER_SIZE = 7, 20, 16, 25
SHAPES = ((10000, 100), (100000, 100))
MIN_SAMPLES = (1, 10)


def stats(ms, digits=4):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], digits), "ms_min": round(ms[0], digits), "ms_max": round(ms[-1], digits)}


def sampled_check(np, x, metric, core, rows, u, v, w):
    """(rows whose smallest float64 weight is not among their tree edges although the runner-up is more than 1e-9 away, tree weights of the rows
    that differ from float64 numpy by more than 1e-9)"""
    X = x.astype(np.float64)
    norms = np.sqrt((X * X).sum(axis=1))
    missing, wrong = 0, 0
    for i in rows:
        if metric == "euclidean":
            dd = np.sqrt(((X - X[i]) ** 2).sum(axis=1))
        else:
            dd = np.maximum(0.0, 1.0 - (X @ X[i]) / (norms * norms[i]))
        if core is not None:
            dd = np.maximum(np.maximum(dd, core), core[i])
        dd[i] = np.inf
        mine = np.nonzero((u == i) | (v == i))[0]
        other = np.where(u[mine] == i, v[mine], u[mine])
        wrong += int((np.abs(w[mine] - dd[other]) > 1e-9).sum())
        first, second = np.partition(dd, 1)[:2]
        missing += int(second - first > 1e-9 and int(np.argmin(dd)) not in other.tolist())
    return missing, wrong


def kernel_ms(ctx, prefix):
    return {v["kernel"]: (v["total_ms"], v["launches"]) for v in ctx.kernel_times() if v["kernel"].startswith(prefix) and v.get("launches")}


def main(path):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    from ganrev import knn
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    res = {"reps": REPS, "silhouette_clusters": CLUSTERS, "min_cluster_size": MIN_CLUSTER_SIZE, "library": os.path.relpath(L.LIB_PATH, ROOT),
           "device": ctx.info(), "rows": []}
    for n, d in SHAPES:
        da = DeviceTensor(ctx, (n, d)); ctx.fill_normal(da.ptr, n * d, 7)
        x = da.numpy()
        labels = np.random.default_rng(n + CLUSTERS).integers(0, CLUSTERS, n).astype(np.int32)
        bufs = [ctx.upload(labels)] + [ctx.malloc(b) for b in (8 * n, 8 * CLUSTERS, 4 * CLUSTERS, 8, 4 * (n - 1), 4 * (n - 1), 8 * (n - 1))]
        lab, sv, cmean, sizes, mean, eu, ev, ew = bufs
        try:
            for metric in ("euclidean", "cosine"):
                for s in MIN_SAMPLES:
                    k = s - 1
                    g = knn.graph(ctx, da, k, metric, keep=True) if k else None
                    try:
                        core_dev = g.dist_dev + 8 * (k - 1) if k else None
                        core = np.ascontiguousarray(g.numpy().dist[:, -1]) if k else None
                        pair, parts, rank, sil, wall, rounds = [], [], [], [], [], []
                        for rep in range(REPS + 1):                     # round 0 is the warm-up
                            ctx.set_timing(2)
                            t0 = time.perf_counter()
                            r = ctx.mst_dev(da.ptr, n, d, metric, core_dev, max(k, 1), eu, ev, ew); ctx.synchronize()
                            took = 1e3 * (time.perf_counter() - t0)
                            a = kernel_ms(ctx, "mst_")
                            ctx.set_timing(0); ctx.set_timing(2)
                            ctx.silhouette_dev(da.ptr, n, d, lab, CLUSTERS, metric, sv, cmean, sizes, mean); ctx.synchronize()
                            b = kernel_ms(ctx, "sil_pair_kernel")
                            ctx.set_timing(0)
                            if rep:
                                (total, launches), = [t for q, t in a.items() if q.startswith("mst_pair_kernel")]
                                assert launches == r
                                pair.append(total / launches); parts.append(a["mst_component_kernels"][0]); rank.append(a["mst_rank_kernel"][0])
                                sil.append(sum(t / q for t, q in b.values())); wall.append(took); rounds.append(r)
                    finally:
                        if g is not None:
                            g.close()
                    u, v, w = ctx.download(eu, (n - 1,), np.int32), ctx.download(ev, (n - 1,), np.int32), ctx.download(ew, (n - 1,), np.float64)
                    host = []
                    for rep in range(REPS):
                        t0 = time.perf_counter()
                        found = L.hdbscan_host(u, v, w, n, MIN_CLUSTER_SIZE)
                        host.append(1e3 * (time.perf_counter() - t0))
                    checked = np.random.default_rng(d + s).choice(n, CHECKED_ROWS, replace=False)
                    missing, wrong = sampled_check(np, x, metric, core, checked, u, v, w)
                    ps, ss = stats(pair), stats(sil)
                    cap = max(1, (n - 1).bit_length())
                    row = {"n": n, "d": d, "metric": metric, "min_samples": s, "mst_pair_kernel_per_round": ps, "sil_pair_kernel": ss,
                           "ratio_of_medians": round(ps["ms_median"] / ss["ms_median"], 3), "ratio_of_minima": round(ps["ms_min"] / ss["ms_min"], 3),
                           "rounds": sorted(set(rounds)), "round_cap": cap, "component_pass_total": stats(parts), "rank_kernel": stats(rank),
                           "call_wall": stats(wall, 2), "hdbscan_host": stats(host, 3), "clusters": found[2], "noise_rows": int((found[0] < 0).sum()),
                           "sorted_and_spanning": bool((np.diff(w) >= 0).all() and (u < v).all() and len(set(u.tolist()) | set(v.tolist())) == n),
                           "checked_rows": CHECKED_ROWS, "nearest_edges_missing": missing, "weights_that_differ_from_numpy": wrong}
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
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_hierarchy.json"))
