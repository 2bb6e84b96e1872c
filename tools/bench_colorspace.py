#!/usr/bin/env python3
"""gr_colorspace_dev (NN_UTILS.switchColorSpace, one fused launch) against gr_copy2d_dev moving the same number of bytes, event-timed on
the context's stream: median and spread of 30 warmed-up launches, achieved bytes/s, for rgb->yuv, yuv->rgb, rgb->hsl, hsl->rgb, y->rgb
and yuv->hsl at 512 x 3 x 64 x 64 and 256 x 3 x 32 x 32.  Then one distillation batch of ganrev.pretrain_with_previous_net
(DeviceDistill, rgb -> yuv, batch 128, f16x3) at 3x32x32 and 3x64x64 in images/s, and the share of the step its two conversions
take (gr_set_timing 2).   python tools/bench_colorspace.py [out.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import models, pretrain_with_previous_net as P
from ganrev.synth import synthetic_images

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
res = {"device": ctx.info(), "conversions": [], "distillation": []}
WARM, REPS = 10, 30
PL = {"rgb": 3, "y": 1, "yuv": 3, "hsl": 3}


def timed(fn):
    for _ in range(WARM):
        fn()
    ms = []
    for i in range(REPS):
        ctx.event_record(2 * i); fn(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    ms = sorted(ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS))
    return ms[REPS // 2], ms[0], ms[-1]


for (n, h, w) in ((512, 64, 64), (256, 32, 32)):
    src, dst = ctx.malloc(4 * n * 3 * h * w), ctx.malloc(4 * n * 3 * h * w)
    ctx.fill_uniform(src, n * 3 * h * w, 1, 0.0, 1.0)
    for f, t in (("rgb", "yuv"), ("yuv", "rgb"), ("rgb", "hsl"), ("hsl", "rgb"), ("y", "rgb"), ("yuv", "hsl")):
        nbytes = 4 * n * h * w * (PL[f] + PL[t])
        med, lo, hi = timed(lambda: ctx.colorspace_dev(src, L.COLOR_SPACES[f], L.COLOR_SPACES[t], n, h, w, dst))
        floats = nbytes // 8                                   # a copy reads and writes: half the bytes each way
        cmed, clo, chi = timed(lambda: ctx.copy2d(dst, floats, src, floats, 1, floats))
        row = {"from": f, "to": t, "shape": [n, 3, h, w], "bytes": nbytes, "ms_median": round(med, 5), "ms_min": round(lo, 5), "ms_max": round(hi, 5),
               "GBps": round(nbytes / med / 1e6, 1), "copy_ms_median": round(cmed, 5), "copy_ms_min": round(clo, 5), "copy_ms_max": round(chi, 5),
               "copy_GBps": round(nbytes / cmed / 1e6, 1), "ratio_to_copy": round(cmed / med, 3)}
        res["conversions"].append(row)
        print(f"{f}->{t} {n}x3x{h}x{w}: {med * 1e3:.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}] {row['GBps']} GB/s; copy of {nbytes} B: "
              f"{cmed * 1e3:.1f} us [{clo * 1e3:.1f}, {chi * 1e3:.1f}] {row['copy_GBps']} GB/s", flush=True)
    ctx.free(src); ctx.free(dst)

B, STEPS = 128, 30
for hw in (32, 64):
    pdims = (3, hw, hw)
    OPT = P.parse(["--batchSize", str(B), "--height", str(hw), "--width", str(hw), "--colorSpace", "yuv", "--quiet"])
    s = P.setup(OPT, models.create_G(pdims, 100, True, 1), models.create_D(pdims, True, 2), (100, "normal", "rgb", hw, hw))
    loop = P.DeviceDistill(s)
    real = synthetic_images(B // 2, pdims, 1)
    for _ in range(WARM):
        loop.batch(real)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        loop.batch(real)
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / STEPS
    ctx.set_timing(2)
    loop.batch(real); ctx.synchronize()
    kt = ctx.kernel_times(); ctx.set_timing(0)
    tot = sum(k["total_ms"] for k in kt)
    cs = [k for k in kt if k["kernel"].startswith("colorspace_kernel")]
    cs_ms, launches = sum(k["total_ms"] for k in cs), sum(k["launches"] for k in cs)
    res["distillation"].append({"dims": list(pdims), "batch": B, "step_ms": round(dt * 1e3, 4), "images_per_s": round(B / dt, 1), "kernel_ms_total": round(tot, 4),
                                "colorspace_launches": launches, "colorspace_ms": round(cs_ms, 5), "colorspace_share_of_kernel_time": round(cs_ms / tot, 5)})
    print(f"distillation {pdims} batch {B}: {dt * 1e3:.3f} ms/step, {B / dt:.0f} images/s; {launches} colour-space launches, {cs_ms * 1e3:.1f} us = "
          f"{100 * cs_ms / tot:.2f} % of the step's kernel time", flush=True)
    loop.close()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_colorspace.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
