#!/usr/bin/env python3
"""One EM iteration of gr_mixture_dev (csrc/mixture.hip) at corpus scale: N = 1 000 000, d = 100 with k = 20, 64 and 256 components, and the default
N = 10 000, d = 32 with k = 20.  Nothing is gated: nobody has measured these times before, and there is no parent to compare with.
Per shape a call with niter = 1 (E-step, M-step, update, and the closing E-step), every kernel under its own pair of events (gr_set_timing 2 /
gr_kernel_times): milliseconds per launch, median [min, max] of 30 calls after one discarded warm-up.  One iteration = one launch each of the
prep, E-step, log-likelihood, M-step and update kernels.  Next to it what an iteration has to move, so the reader sees the distance to the roofline:
   bytes          two passes over the table, 2 x 4 N d, at the 8 TB/s HBM rate DESIGN.md uses
   multiply-adds  two dense passes, 2 N k d (the log-densities, the moment sums)
   fp64 floor     the library spends 15 separately rounded fp64 operations per (row, component, column) - 4 for the E-step's log-density, 4 to
                  recompute it in the M-step (the responsibilities are never stored), 7 for the three moment chains - at the fp64 vector peak of
                  78.6 TFLOP/s, which counts a fused multiply-add as two: 39.3 T separately rounded operations per second
   python tools/bench_mixture.py [out.json]      # -> profiles/bench_mixture.json"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, HBM, FP64_UNFUSED, OPS_PER_TERM = 30, 8.0e12, 78.6e12 / 2, 15
SHAPES = ((1000000, 100, 20), (1000000, 100, 64), (1000000, 100, 256), (10000, 32, 20))
PER_ITERATION = ("mix_prep_kernel", "mix_estep_kernel", "mix_loglik_kernels", "mix_mstep_kernel", "mix_update_kernel")


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def main(path):
    sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
    import numpy as np
    import ganrev._lib as L
    from ganrev.nn_utils import DeviceTensor
    ctx = L.default_context()
    res = {"reps": REPS, "hbm_bytes_per_s": HBM, "fp64_unfused_ops_per_s": FP64_UNFUSED, "fp64_ops_per_row_component_column": OPS_PER_TERM,
           "library": os.path.relpath(L.LIB_PATH, ROOT), "device": ctx.info(), "rows": []}
    for N, d, k in SHAPES:
        da = DeviceTensor(ctx, (N, d)); ctx.fill_normal(da.ptr, N * d, 7)
        means0 = ctx.download(da.ptr, (k, d)).copy()                   # the first k rows: distinct, inside the cloud
        w0, var0 = np.full(k, 1.0 / k, np.float32), np.ones((k, d), np.float32)
        bufs = [ctx.upload(a) for a in (w0, means0, var0)] + [ctx.malloc(16)]
        w, mu, var, ll = bufs
        per = {}
        try:
            for rep in range(REPS + 1):
                for src, dst in ((w0, w), (means0, mu), (var0, var)):
                    ctx.upload(src, dst)
                ctx.set_timing(2)
                ctx.mixture_dev(da.ptr, N, d, k, 1, 1e-3, w, mu, var, ll); ctx.synchronize()
                kt = {v["kernel"]: v for v in ctx.kernel_times() if v["kernel"].startswith("mix_") and v.get("launches")}
                ctx.set_timing(0)
                assert set(kt) == set(PER_ITERATION), sorted(kt)
                if rep:                                                 # repetition 0 is the warm-up
                    for name, v in kt.items():
                        per.setdefault(name, []).append(v["total_ms"] / v["launches"])
                    per.setdefault("iteration", []).append(sum(kt[name]["total_ms"] / kt[name]["launches"] for name in PER_ITERATION))
            loglik = ctx.download(ll, (2,), np.float64)
        finally:
            for b in bufs:
                ctx.free(b)
            da.free()
        stream_ms, fp64_ms = 2 * 4.0 * N * d / HBM * 1e3, float(OPS_PER_TERM) * N * d * k / FP64_UNFUSED * 1e3
        floor_ms = max(stream_ms, fp64_ms)
        row = {"n": N, "d": d, "k": k, "bytes_per_iteration": 2 * 4 * N * d, "multiply_adds_per_iteration": 2 * N * d * k,
               "streaming_floor_ms": round(stream_ms, 4), "fp64_floor_ms": round(fp64_ms, 4), "floor": "streaming" if stream_ms >= fp64_ms else "fp64",
               "kernels_ms_per_launch": {name: stats(v) for name, v in per.items() if name != "iteration"},
               "iteration_ms": dict(stats(per["iteration"]), x_floor=round(stats(per["iteration"])["ms_median"] / floor_ms, 2)),
               "loglik": [float(v) for v in loglik]}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_mixture.json"))
