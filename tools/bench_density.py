#!/usr/bin/env python3
"""gr_eps_graph_dev and gr_dbscan_dev (csrc/density.hip) at corpus scale: bench_knn.py's shapes (n, d) = (10 000, 100) and (100 000, 100), under
both distances, minPts 10, eps the 0.75-quantile of the rows' distances to their 9th neighbour (density.epsFromNeighbours).  Beside the eps-graph's
pair kernel stands the yardstick: gr_silhouette_dev's pair kernel on the same table with 20 clusters - the same pair arithmetic, with 64 ordered
adds per row and tile where the eps-graph has 64 compares, four shuffles and one store.  Both are timed in one process, in alternating calls (one
eps-graph, one silhouette, seven times after one discarded round), every kernel under its own pair of events (gr_set_timing 2 /
gr_kernel_times): milliseconds per launch, median [min, max].  The ratio eps_pair_kernel / sil_pair_kernel is what DESIGN.md expects at or below
1.  gr_dbscan_dev is timed on the finished bitmap the same way: its rounds (launches of the round kernels) and the sum of its kernels, and the
wall time of the call with its stream waits.  The table is Gaussian noise.
Each bitmap is also checked where it was measured: 16 rows' neighbourhoods against float64 numpy, away from eps by more than 1e-9.
   python tools/bench_density.py [out.json]      # -> profiles/bench_density.json"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, CLUSTERS, CHECKED_ROWS, MIN_PTS, QUANTILE = 7, 20, 16, 10, 0.75
SHAPES = ((10000, 100), (100000, 100))


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def sampled_check(np, x, metric, eps, rows, words, count):
    """(bits that differ from float64 numpy's among the pairs more than 1e-9 away from eps, rows whose count differs when no pair of theirs is that close)"""
    X = x.astype(np.float64)
    norms = np.sqrt((X * X).sum(axis=1))
    wrong, wrong_counts = 0, 0
    for i in rows:
        if metric == "euclidean":
            dd = np.sqrt(((X - X[i]) ** 2).sum(axis=1))
        else:
            dd = np.maximum(0.0, 1.0 - (X @ X[i]) / (norms * norms[i]))
        want = dd <= eps
        want[i] = True
        got = np.unpackbits(words[i].view(np.uint8), bitorder="little")[:len(X)].astype(bool)
        clear = np.abs(dd - eps) > 1e-9
        wrong += int((got != want)[clear].sum())
        wrong_counts += int(clear.all() and int(want.sum()) != int(count[i]))
    return wrong, wrong_counts


def kernel_ms(ctx, prefix):
    return {v["kernel"]: (v["total_ms"], v["launches"]) for v in ctx.kernel_times() if v["kernel"].startswith(prefix) and v.get("launches")}


def main(path):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    from ganrev import density
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    res = {"reps": REPS, "silhouette_clusters": CLUSTERS, "min_pts": MIN_PTS, "quantile": QUANTILE, "library": os.path.relpath(L.LIB_PATH, ROOT),
           "device": ctx.info(), "rows": []}
    for n, d in SHAPES:
        da = DeviceTensor(ctx, (n, d)); ctx.fill_normal(da.ptr, n * d, 7)
        x = da.numpy()
        labels = np.random.default_rng(n + CLUSTERS).integers(0, CLUSTERS, n).astype(np.int32)
        words = L.Context.eps_words(n)
        bufs = [ctx.upload(labels)] + [ctx.malloc(b) for b in (8 * n, 8 * CLUSTERS, 4 * CLUSTERS, 8, 8 * n * words, 4 * n, 4 * n, 4 * n, 4)]
        lab, sv, cmean, sizes, mean, adj, count, out_labels, out_core, out_clusters = bufs
        try:
            for metric in ("euclidean", "cosine"):
                eps, kdist = density.epsFromNeighbours(ctx, da, MIN_PTS, QUANTILE, metric)
                graph, sil, scan, scan_wall, rounds = [], [], [], [], []
                for rep in range(REPS + 1):                             # round 0 is the warm-up
                    ctx.set_timing(2)
                    ctx.eps_graph_dev(da.ptr, n, d, eps, metric, adj, count); ctx.synchronize()
                    a = kernel_ms(ctx, "eps_pair_kernel")
                    ctx.set_timing(0); ctx.set_timing(2)
                    ctx.silhouette_dev(da.ptr, n, d, lab, CLUSTERS, metric, sv, cmean, sizes, mean); ctx.synchronize()
                    b = kernel_ms(ctx, "sil_pair_kernel")
                    ctx.set_timing(0); ctx.set_timing(2)
                    t0 = time.perf_counter()
                    ctx.dbscan_dev(adj, count, n, MIN_PTS, out_labels, out_core, out_clusters); ctx.synchronize()
                    wall = 1e3 * (time.perf_counter() - t0)
                    c = kernel_ms(ctx, "dbscan_")
                    ctx.set_timing(0)
                    if rep:
                        graph.append(sum(t / k for t, k in a.values())); sil.append(sum(t / k for t, k in b.values()))
                        scan.append(sum(t for t, _ in c.values())); scan_wall.append(wall); rounds.append(c["dbscan_round_kernels"][1])
                host_words, host_count = ctx.download(adj, (n, words), np.uint64), ctx.download(count, (n,), np.int32)
                got = ctx.download(out_labels, (n,), np.int32)
                core = ctx.download(out_core, (n,), np.int32).astype(bool)
                checked = np.random.default_rng(d).choice(n, CHECKED_ROWS, replace=False)
                wrong, wrong_counts = sampled_check(np, x, metric, eps, checked, host_words, host_count)
                gs, ss = stats(graph), stats(sil)
                row = {"n": n, "d": d, "metric": metric, "eps": eps, "eps_pair_kernel": gs, "sil_pair_kernel": ss,
                       "ratio_of_medians": round(gs["ms_median"] / ss["ms_median"], 3), "ratio_of_minima": round(gs["ms_min"] / ss["ms_min"], 3),
                       "dbscan_rounds": sorted(set(rounds)), "dbscan_kernels_total": stats(scan), "dbscan_call_wall": stats(scan_wall),
                       "clusters": int(ctx.download(out_clusters, (1,), np.int32)[0]), "core_rows": int(core.sum()), "noise_rows": int((got < 0).sum()),
                       "core_rows_equal_kdist_within_eps": bool(np.array_equal(core, kdist <= eps)),
                       "checked_rows": CHECKED_ROWS, "bits_that_differ_from_numpy": wrong, "counts_that_differ_from_numpy": wrong_counts}
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
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_density.json"))
