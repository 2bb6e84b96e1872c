#!/usr/bin/env python3
"""pretrain_g.lua's autoencoder step (ganrev.pretrain_g.DeviceLoop: forward, MSE, backward, penalty-clamp-Adam) in images/s at
3x32x32 and 3x64x64, batch 128, f16x3, warmed up and device-synchronised; the per-kernel table of one step (gr_set_timing 2); and
the average-pool pipeline kernels against the max-pool kernels on the same tensor (one conv - BN - ReLU - pool stage, training
forward + backward).   python tools/bench_pretrain_g.py [out.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import nn, pretrain_g, synth
from ganrev.synth import synthetic_images

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
res = {"device": ctx.info(), "conv_mode": "f16x3", "autoencoder": [], "pool_kernels": []}
B, STEPS, WARM = 128, 50, 10
for dims in ((3, 32, 32), (3, 64, 64)):
    ae = pretrain_g.build(dims, 100, 1); ae._ctx = ctx
    loop = pretrain_g.DeviceLoop(ae, dims, B, L.Hyper(l1=0.0, l2=0.0, clamp=5.0))
    loop.load(synthetic_images(B * 4, dims, 1))
    for i in range(WARM):
        loop.batch(i % 4)
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(STEPS):
        loop.batch(i % 4)
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / STEPS
    ctx.set_timing(2)
    loop.batch(0); ctx.synchronize()
    kt = ctx.kernel_times(); ctx.set_timing(0)
    table = sorted(({"kernel": k["kernel"], "launches": k["launches"], "ms": round(k["total_ms"], 4)} for k in kt), key=lambda r: -r["ms"])
    res["autoencoder"].append({"dims": list(dims), "batch": B, "step_ms": round(dt * 1e3, 4), "images_per_s": round(B / dt, 1), "kernels": table})
    print(f"autoencoder {dims} batch {B}: {dt * 1e3:.3f} ms/step, {B / dt:.0f} images/s", flush=True)
    loop.close()

# the same tensor through the max-pool and the average-pool pipeline kernels: conv 64 -> 64 at 32x32 (the float4 kernels)
# and at 64x64 with 128 images; pipeline kernels only (post_*), median of 5 timed iterations
for (Bp, C, H) in ((128, 64, 32), (64, 64, 64)):
    x = synth.uniform((Bp, C, H, H), 3, -1, 1); gy = None
    for pool in ("max", "avg"):
        m = nn.Sequential(); m.add(nn.SpatialConvolution(C, C)); m.add(nn.SpatialBatchNormalization(C)); m.add(nn.ReLU())
        m.add(nn.SpatialMaxPooling(2, 2) if pool == "max" else nn.SpatialAveragePooling(2, 2, 2, 2))
        synth.init_params(m, 2); m.training()
        out = m.forward(x)
        gy = synth.normal(out.shape, 4) if gy is None else gy
        m.backward(x, gy)
        per = {}
        for _ in range(5):
            ctx.set_timing(2)
            m.forward(x); m.backward(x, gy); ctx.synchronize()
            for k in ctx.kernel_times():
                if k["kernel"].startswith("post_"):
                    per.setdefault(k["kernel"], []).append(k["total_ms"])
            ctx.set_timing(0)
        row = {"pool": pool, "batch": Bp, "C": C, "H": H, "W": H, "kernels_ms": {k: round(float(np.median(v)), 4) for k, v in sorted(per.items())}}
        res["pool_kernels"].append(row)
        print(f"{pool} pool B={Bp} C={C} {H}x{H}: " + "; ".join(f"{k} {v * 1e3:.1f} us" for k, v in row["kernels_ms"].items()), flush=True)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_pretrain_g.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
