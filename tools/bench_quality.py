#!/usr/bin/env python3
"""What scoring a table of reconstructions costs: gr_ssim_dev (SSIM, MSE and the mean in one call, 11 x 11 Gaussian window) over
10 000 x 3x32x32, 10 000 x 3x64x64 and 1 000 000 x 1x32x32, and gr_mse_rows_dev over the same tables beside it - the bandwidth-bound yardstick: it
reads the same 8 bytes a pixel and does three operations on them, where the SSIM does some 200 in fp64.  Tables filled on the device (uniform in
[0, 1]).  Event-timed on the context's stream, median [min, max] of 30 after one discarded warm-up.  No time is asserted anywhere.
    python tools/bench_quality.py [out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import ganrev._lib as L

ctx = L.default_context()
REPS, WIN, SIGMA = 30, 11, 1.5
res = {"device": ctx.info(), "reps": REPS, "win": WIN, "sigma": SIGMA, "cases": []}


def timed(fn):
    fn()                                                       # the warm-up, discarded
    for i in range(REPS):
        ctx.event_record(2 * i); fn(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    ms = sorted(ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS))
    return {"ms_median": round(ms[REPS // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


for n, c, h, w in ((10000, 3, 32, 32), (10000, 3, 64, 64), (1000000, 1, 32, 32)):
    per = c * h * w
    a, b = ctx.malloc(4 * n * per), ctx.malloc(4 * n * per)
    rows, mse, mean = ctx.malloc(4 * n), ctx.malloc(4 * n), ctx.malloc(8)
    try:
        ctx.fill_uniform(a, n * per, 1, 0.0, 1.0); ctx.fill_uniform(b, n * per, 2, 0.0, 1.0)
        row = {"n": n, "dims": [c, h, w], "table_bytes": 8 * n * per}
        row["ssim_dev"] = timed(lambda: ctx.ssim_dev(a, b, n, c, h, w, rows, mse, mean, win=WIN, sigma=SIGMA))
        row["ssim_dev_rows_only"] = timed(lambda: ctx.ssim_dev(a, b, n, c, h, w, rows, None, None, win=WIN, sigma=SIGMA))
        row["mse_rows_dev"] = timed(lambda: ctx.mse_rows_dev(a, b, n, per, mse))
        row["mse_rows_GBps"] = round(row["table_bytes"] / row["mse_rows_dev"]["ms_median"] / 1e6, 1)
        row["ssim_over_mse_rows"] = round(row["ssim_dev"]["ms_median"] / row["mse_rows_dev"]["ms_median"], 2)
        oh, ow = h - WIN + 1, w - WIN + 1
        row["ssim_fp64_Gops"] = round(n * c * 20.0 * WIN * (h * ow + oh * ow) / row["ssim_dev"]["ms_median"] / 1e6, 1)      # multiplies and adds of the two passes
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    finally:
        for p in (a, b, rows, mse, mean):
            ctx.free(p)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_quality.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
