#!/usr/bin/env python3
"""The clustering of apply_r.lua:197-243 at corpus scale: 15 k-means iterations with k = 20 at N = 1 000 000, d = 100 and at N = 10 000, d = 32.
Two arms, each in a process of its own because the library is chosen when the package loads:
   base   the parent commit's library (tools/build_base.sh -> tools/probe/libganrev_base.so), through gr_kmeans_host
   new    the working tree's library, through gr_kmeans_dev
Per arm: the k-means kernels that read the table, each launch under its own pair of events (gr_set_timing 2 / gr_kernel_times), as milliseconds
per iteration, median [min, max] of 30 calls after one discarded warm-up, next to the streaming floor of one pass, 4 N d bytes at the 8 TB/s HBM
rate DESIGN.md uses.  And the wall time of the whole clustering step (apply_r.createClusterImagesDev, 71 rows per cluster, 1 x 8 x 8 images):
base from the host attribute table (upload, k-means, download, upload, assignment, download, numpy selection, one gr_rows_mean_dev per
cluster), new from the device table (gr_kmeans_dev + gr_cosine_assign_dev + gr_cluster_members_dev + gr_cluster_faces_dev), median of 7.
   tools/build_base.sh <parent rev>   # e.g. HEAD~1 once this change is committed: the base arm's library
   python tools/bench_cluster.py [out.json]
More than 32 clusters (gr_cluster_dev; the parent cannot run them, so there is no base arm):
   python tools/bench_cluster.py --wide [out.json]      # -> profiles/bench_cluster_wide.json
k = 32 on the narrow route and forced onto the wide one ("cluster_wide_min_k" 1), then 64, 256, 1024 and 4096, at the same two shapes, 15 iterations,
71 rows per cluster: every kernel of the call under its own events, per launch, median [min, max] of 30 calls after a warm-up; the k-means kernels'
sum per iteration against the larger of two floors - streaming 4 N d bytes at 8 TB/s, and 2 N d k unfused multiplies and adds at the vector peak
(157.3 TFLOP/s counts a fused multiply-add as two operations: 78.65 T separately rounded ones per second)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_LIB = os.path.join(ROOT, "tools", "probe", "libganrev_base.so")
NEW_SYMBOLS = ("gr_kmeans_dev", "gr_cosine_assign_dev", "gr_cluster_members_dev", "gr_cluster_faces_dev")
REPS, WALL_REPS, ITERS, K, HBM = 30, 7, 15, 20, 8.0e12
SHAPES = ((1000000, 100), (10000, 32))


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def arm(name):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    if name == "base":                                  # the parent's library does not export them
        for s in NEW_SYMBOLS:
            L._SIGS.pop(s, None)
    from ganrev import apply_r
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    out = {"arm": name, "library": os.path.relpath(L.LIB_PATH, ROOT), "device": ctx.info(), "shapes": []}
    for N, d in SHAPES:
        da = DeviceTensor(ctx, (N, d)); ctx.fill_normal(da.ptr, N * d, 7)
        di = DeviceTensor(ctx, (N, 1, 8, 8)); ctx.fill_normal(di.ptr, N * 64, 8)
        x = da.numpy()
        c0 = apply_r.initialCentroids(K, d, 1)
        cent, lab = ctx.upload(c0), ctx.malloc(4 * N)

        def kmeans():
            if name == "base":
                return ctx.kmeans(x, K, ITERS, c0)
            ctx.upload(c0, cent)
            ctx.kmeans_dev(da.ptr, N, d, K, ITERS, cent, None, lab)
        per = {}
        for rep in range(REPS + 1):
            ctx.set_timing(2)
            kmeans(); ctx.synchronize()
            kt = {k["kernel"]: k for k in ctx.kernel_times() if k["kernel"].startswith("kmeans_") and k.get("launches")}
            ctx.set_timing(0)
            assert kt and all(k["launches"] == ITERS for k in kt.values()), kt
            if rep:                                     # repetition 0 is the warm-up
                for k, v in kt.items():
                    per.setdefault(k, []).append(v["total_ms"] / ITERS)
                per.setdefault("per_iteration", []).append(sum(v["total_ms"] for v in kt.values()) / ITERS)
        floor_ms = 4.0 * N * d / HBM * 1e3
        row = {"n": N, "d": d, "k": K, "iterations": ITERS, "streaming_floor_ms_per_pass": round(floor_ms, 4), "kernels_ms_per_iteration": {}}
        for k, v in per.items():
            row["kernels_ms_per_iteration"][k] = dict(stats(v), x_floor=round(stats(v)["ms_median"] / floor_ms, 2))
        wall = []
        for rep in range(WALL_REPS + 1):
            ctx.synchronize(); t0 = time.perf_counter()
            res = apply_r.createClusterImagesDev(K, ITERS, 71, di, x if name == "base" else da, centroids0=c0)
            ctx.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
            res[3].free()
        row["cluster_step_wall"] = dict(stats(wall[1:]), reps=WALL_REPS, route="host table" if name == "base" else "device table")
        row["centroid_checksum"] = float(np.asarray(res[0], np.float64).sum())          # the two arms compute the same bits
        out["shapes"].append(row)
        print(json.dumps(row), flush=True)
        for p in (cent, lab):
            ctx.free(p)
        da.free(); di.free()
    print("ARM " + json.dumps(out), flush=True)


WIDE_KS = ((32, False), (32, True), (64, False), (256, False), (1024, False), (4096, False))      # (k, forced onto the wide route)
VALU_UNFUSED = 157.3e12 / 2


def wide(path):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    from ganrev import apply_r
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    M = 71
    res = {"reps": REPS, "iterations": ITERS, "rows_per_cluster": M, "hbm_bytes_per_s": HBM, "valu_unfused_ops_per_s": VALU_UNFUSED,
           "library": os.path.relpath(L.LIB_PATH, ROOT), "device": ctx.info(), "rows": []}
    for N, d in SHAPES:
        da = DeviceTensor(ctx, (N, d)); ctx.fill_normal(da.ptr, N * d, 7)
        for k, forced in WIDE_KS:
            c0 = apply_r.initialCentroids(k, d, 1)
            bufs = [ctx.upload(c0)] + [ctx.malloc(b) for b in (4 * k, 4 * N, 4 * N, 8 * k * M, 4 * k * M, 4 * k, 4 * k)]
            cent, tot, lab, sim, rows, rsim, kept, csize = bufs
            ctx.set_tuning("cluster_wide_min_k", 1 if forced else L.Context.CLUSTER_WIDE_MIN_K)
            per, call = {}, []
            try:
                for rep in range(REPS + 1):
                    ctx.upload(c0, cent)
                    ctx.set_timing(2)
                    ctx.cluster_dev(da.ptr, N, d, k, ITERS, cent, True, M, tot, lab, sim, rows, rsim, kept, csize); ctx.synchronize()
                    kt = {v["kernel"]: v for v in ctx.kernel_times() if v.get("launches")}
                    ctx.set_timing(0)
                    if rep:                             # repetition 0 is the warm-up
                        for name, v in kt.items():
                            per.setdefault(name, []).append(v["total_ms"] / v["launches"])
                        km = [v["total_ms"] for name, v in kt.items() if name.startswith("kmeans_") or name == "wide_segment_sum_kernel"]
                        grp = kt.get("wide_group_kernel")
                        per.setdefault("kmeans_per_iteration", []).append((sum(km) + (grp["total_ms"] * ITERS / grp["launches"] if grp else 0.0)) / ITERS)
                        call.append(sum(v["total_ms"] for v in kt.values()))
                launches = {name: v["launches"] for name, v in kt.items()}
                checksum = float(np.asarray(ctx.download(cent, (k, d)), np.float64).sum())
            finally:
                ctx.set_tuning("cluster_wide_min_k", L.Context.CLUSTER_WIDE_MIN_K)
                for b in bufs:
                    ctx.free(b)
            stream_ms, valu_ms = 4.0 * N * d / HBM * 1e3, 2.0 * N * d * k / VALU_UNFUSED * 1e3
            floor_ms = max(stream_ms, valu_ms)
            row = {"n": N, "d": d, "k": k, "route": "wide" if forced or k >= L.Context.CLUSTER_WIDE_MIN_K else "narrow", "forced": forced,
                   "streaming_floor_ms": round(stream_ms, 4), "valu_floor_ms": round(valu_ms, 4), "floor": "streaming" if stream_ms >= valu_ms else "valu",
                   "launches_per_call": launches, "kernels_ms_per_launch": {}, "kernels_ms_per_call_sum": stats(call), "centroid_checksum": checksum}
            for name, v in per.items():
                row["kernels_ms_per_launch"][name] = dict(stats(v), x_floor=round(stats(v)["ms_median"] / floor_ms, 2))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        da.free()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if len(sys.argv) > 1 and sys.argv[1] == "--wide":
    wide(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bench_cluster_wide.json"))
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[1] == "--arm":
    arm(sys.argv[2])
    sys.exit(0)
if not os.path.exists(BASE_LIB):
    sys.exit(f"{BASE_LIB} is missing: build the parent commit's library with tools/build_base.sh <parent> first")
res = {"reps": REPS, "hbm_bytes_per_s": HBM}
for name in ("base", "new"):
    env = dict(os.environ)
    if name == "base":
        env["GANREV_LIB"] = BASE_LIB
    else:
        env.pop("GANREV_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", name], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    print(p.stdout, end="", flush=True)
    if p.returncode:
        sys.exit(f"arm {name} ended with status {p.returncode}")
    res[name] = json.loads([l for l in p.stdout.splitlines() if l.startswith("ARM ")][-1][4:])
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_cluster.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
