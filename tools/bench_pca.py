#!/usr/bin/env python3
"""The three stages of ganrev.pca at corpus scale: the table of cfg5 (1 000 000 x 100) and a wide one (100 000 x 256).
   covariance   pca_mean_kernel + pca_cov_kernel (two passes over the table, their joins included)
   eigen        pca_jacobi_kernel (ONE workgroup by design)
   projection   pca_project_kernel, onto 2 axes (the map of a corpus) and onto all d (the whitened table)
Every kernel under its own pair of events (gr_set_timing 2 / gr_kernel_times): milliseconds, median [min, max] of 30 calls after one discarded
warm-up, next to the floor of one streaming read of the table (4 n d bytes at the 8 TB/s HBM rate DESIGN.md uses; README measures the exact
five-needle search over 1 M x 100 at 0.13-0.14 ms) and to numpy float64 on the same host (np.cov + np.linalg.eigh, 16 threads, median of 3).
   python tools/bench_pca.py [out.json]      # -> profiles/bench_pca.json"""
import json, os, sys, time
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
REPS, NUMPY_REPS, HBM = 30, 3, 8.0e12
SHAPES = ((1000000, 100), (100000, 256))
STAGES = {"covariance": ("pca_mean_kernel", "pca_cov_kernel"), "eigen": ("pca_jacobi_kernel",), "projection": ("pca_project_kernel",)}


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def timed(ctx, call, names):
    """-> {kernel: [ms per call]} over REPS calls after a warm-up"""
    per = {}
    for rep in range(REPS + 1):
        ctx.set_timing(2)
        call(); ctx.synchronize()
        kt = {v["kernel"]: v for v in ctx.kernel_times() if v["kernel"] in names and v.get("launches")}
        ctx.set_timing(0)
        assert sorted(kt) == sorted(names), kt
        if rep:                                         # repetition 0 is the warm-up
            for name, v in kt.items():
                per.setdefault(name, []).append(v["total_ms"])
    return per


def main(path):
    import numpy as np
    import ganrev._lib as L
    from ganrev import pca as P
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    res = {"reps": REPS, "hbm_bytes_per_s": HBM, "library": os.path.relpath(L.LIB_PATH, ROOT), "device": ctx.info(), "numpy_threads": os.environ["OMP_NUM_THREADS"], "rows": []}
    for n, d in SHAPES:
        da = DeviceTensor(ctx, (n, d)); ctx.fill_normal(da.ptr, n * d, 7)
        pca = P.principalAxes(ctx, da.ptr, n, d)
        floor_ms = 4.0 * n * d / HBM * 1e3
        row = {"n": n, "d": d, "sweeps": pca.sweeps, "converged": pca.converged, "streaming_floor_ms_per_pass": round(floor_ms, 4), "stages": {}}
        per = timed(ctx, lambda: ctx.pca_dev(da.ptr, n, d, pca.mean_dev, pca.cov_dev, pca.eigvals_dev, pca.axes_dev, pca.info_dev), STAGES["covariance"] + STAGES["eigen"])
        for stage in ("covariance", "eigen"):
            total = [sum(v) for v in zip(*(per[k] for k in STAGES[stage]))]
            row["stages"][stage] = dict(stats(total), x_floor=round(stats(total)["ms_median"] / floor_ms, 2), kernels={k: stats(per[k]) for k in STAGES[stage]})
        for k in (2, d):
            out = DeviceTensor(ctx, (n, k))
            per = timed(ctx, lambda: ctx.pca_project_dev(da.ptr, n, d, pca.mean_dev, pca.axes_dev, pca.eigvals_dev, k, True, out.ptr), STAGES["projection"])
            v = per["pca_project_kernel"]
            row["stages"]["projection_k%d" % k] = dict(stats(v), x_floor=round(stats(v)["ms_median"] / floor_ms, 2))
            out.free()
        x = da.numpy()
        wall = []
        for _ in range(NUMPY_REPS):
            t0 = time.perf_counter()
            w, v = np.linalg.eigh(np.cov(x, rowvar=False, dtype=np.float64))
            wall.append((time.perf_counter() - t0) * 1e3)
        row["numpy_float64_cov_eigh"] = dict(stats(wall), reps=NUMPY_REPS)
        row["eigenvalue_max_rel_diff_to_numpy"] = float(np.abs(pca.eigenvalues - w[::-1]).max() / np.abs(w).max())
        row["jacobi_longer_than_covariance"] = row["stages"]["eigen"]["ms_median"] > row["stages"]["covariance"]["ms_median"]
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        pca.close(); da.free()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_pca.json"))
