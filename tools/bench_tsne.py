#!/usr/bin/env python3
"""Exact t-SNE on the device (ganrev.tsne) at n = 2048, 10000 and 16384 rows, d = 32 and 100:
   affinities   gr_tsne_affinities_dev once per map: tsne_cond_kernel (distances + the search on beta, the transpose before it included) and
                tsne_symm_kernel
   iteration    one gr_tsne_gradient_dev + gr_tsne_update_dev: tsne_pass_kernel (reads P once), tsne_combine_kernel, tsne_update_kernel (the
                re-centring included)
Every kernel under its own pair of events (gr_set_timing 2 / gr_kernel_times): milliseconds, median [min, max] of 30 calls after one discarded
warm-up.  The bytes of P the pass reads (4 n^2) per second stand next to the HBM peak (8 TB/s spec, 6.29 TB/s measured for a float4 copy);
P at n = 2048 (16 MiB) fits the L2s and at n = 10000 (400 MB) not even the Infinity Cache.  1000 iterations through gr_tsne_run_dev are timed on
the host clock around one call and one synchronisation.  Baseline: the float64 numpy twin (tests/tsne_oracle.py, matrix form, 16 threads) at
n = 2048, seconds per iteration over 5 iterations.
   python tools/bench_tsne.py [out.json]      # -> profiles/bench_tsne.json"""
import json, os, sys, time
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), os.path.join(ROOT, "tests"), ROOT]
REPS, HBM_SPEC, HBM_COPY = 30, 8.0e12, 6.29e12
SIZES, DIMS = (2048, 10000, 16384), (32, 100)
AFFINITY_KERNELS, ITERATION_KERNELS = ("tsne_cond_kernel", "tsne_symm_kernel"), ("tsne_pass_kernel", "tsne_combine_kernel", "tsne_update_kernel")


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


def staged(per, names):
    total = [sum(v) for v in zip(*(per[k] for k in names))]
    return dict(stats(total), kernels={k: stats(per[k]) for k in names})


def main(path):
    import numpy as np
    import ganrev._lib as L
    from ganrev import device
    import tsne_oracle as to
    ctx = L.default_context()
    res = {"reps": REPS, "hbm_spec_bytes_per_s": HBM_SPEC, "hbm_float4_copy_bytes_per_s": HBM_COPY, "library": os.path.relpath(L.LIB_PATH, ROOT),
           "device": ctx.info(), "numpy_threads": os.environ["OMP_NUM_THREADS"], "rows": []}
    for n in SIZES:
        mem = device.Buffers(ctx)
        try:
            p, beta, info = mem.malloc(4 * n * n), mem.malloc(8 * n), mem.malloc(8)
            y, grad, inc, gains = (mem.malloc(8 * n) for _ in range(4))
            row = {"n": n, "p_bytes": 4 * n * n, "affinities": {}}
            for d in DIMS:
                x = mem.malloc(4 * n * d); ctx.fill_normal(x, n * d, 7)
                per = timed(ctx, lambda: ctx.tsne_affinities_dev(x, n, d, 30.0, p, beta, info), AFFINITY_KERNELS)
                hinfo = ctx.download(info, (2,), np.int32)
                row["affinities"]["d%d" % d] = dict(staged(per, AFFINITY_KERNELS), beta_updates_max=int(hinfo[0]), beta_capped_rows=int(hinfo[1]))
                mem.free(x)
            # the iteration does not see d: P of the last table, a layout in the middle of a run
            ctx.upload(to.layout(n, 1.0), y); ctx.upload(np.zeros((n, 2), np.float32), inc); ctx.upload(np.ones((n, 2), np.float32), gains)

            def iteration():
                ctx.tsne_gradient_dev(p, y, n, 1.0, grad)
                ctx.tsne_update_dev(y, grad, inc, gains, n, 1e-3, 0.8, 0.01)      # (a tiny eta: 31 steps leave the layout where it is)
            per = timed(ctx, iteration, ITERATION_KERNELS)
            it = staged(per, ITERATION_KERNELS)
            pass_ms = it["kernels"]["tsne_pass_kernel"]["ms_median"]
            it.update(p_bytes_per_s=round(4.0 * n * n / (pass_ms * 1e-3)), of_hbm_spec=round(4.0 * n * n / (pass_ms * 1e-3) / HBM_SPEC, 3),
                      of_hbm_float4_copy=round(4.0 * n * n / (pass_ms * 1e-3) / HBM_COPY, 3),
                      longest_kernel=max(ITERATION_KERNELS, key=lambda k: it["kernels"][k]["ms_median"]))
            row["iteration"] = it
            cfg = L.TsneConfig(eta=max(n / 12.0, 50.0))
            ctx.upload(to.layout(n, 1e-4), y); ctx.upload(np.zeros((n, 2), np.float32), inc); ctx.upload(np.ones((n, 2), np.float32), gains)
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.tsne_run_dev(p, n, cfg, y, inc, gains, 0, 1000, None, 0); ctx.synchronize()
            row["run_1000_iterations_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            row["run_1000_final_layout_finite"] = bool(np.isfinite(ctx.download(y, (n, 2))).all())
            if n == SIZES[0]:
                P = ctx.download(p, (n, n)).astype(np.float64)
                t0 = time.perf_counter()
                to.run(P, to.layout(n, 1e-4), 5, max(n / 12.0, 50.0))
                row["numpy_float64_twin_ms_per_iteration"] = round((time.perf_counter() - t0) * 1e3 / 5, 2)
        finally:
            mem.close()
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_tsne.json"))
