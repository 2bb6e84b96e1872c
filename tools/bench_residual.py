#!/usr/bin/env python3
"""The pointwise convolution (csrc/conv1x1.hip) and a models.createResidual block at batch 256, 32x32: the three passes of
nn.SpatialConvolution(Cin, Cout, 1,1,1,1,0,0) at 64 -> 32 and 32 -> 64 planes, each kernel under its own pair of events
(gr_set_timing 2, one forward + backward per repetition), and createResidual(64, 32, 64) forward + backward through
device.DeviceModel, event-timed on the context's stream.  Median [min, max] of 30 after one discarded warm-up.  Next to every
kernel: its streaming floor, 4 B HW (Cin + Cout) bytes at the 8 TB/s HBM rate DESIGN.md uses.
   python tools/bench_residual.py [out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import device, models, synth

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
REPS, B, H, W, HBM = 30, 256, 32, 32, 8.0e12
res = {"device": ctx.info(), "reps": REPS, "batch": B, "hw": [H, W], "hbm_bytes_per_s": HBM, "operator": [], "block": None}
KERNELS = ("conv1x1_kernel", "conv1x1_kernel(dgrad)", "conv1x1_wgrad_kernel", "conv1x1_wgrad_reduce_kernel")


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


for cin, cout in ((64, 32), (32, 64)):
    net = L.Net(ctx, [(L.CONVK, cin, cout, 1, 0.0, 0)], (cin, H, W))
    net.set_params(synth.uniform((net.n_params,), 1, -0.1, 0.1))
    x, g = ctx.malloc(4 * B * cin * H * W), ctx.malloc(4 * B * cout * H * W)
    gin = ctx.malloc(4 * B * cin * H * W)
    ctx.fill_normal(x, B * cin * H * W, 2); ctx.fill_normal(g, B * cout * H * W, 3)
    per = {k: [] for k in KERNELS}
    for rep in range(REPS + 1):
        ctx.set_timing(2)
        net.forward_dev(x, B); net.backward_dev(x, g, B, gin)
        ctx.synchronize()
        kt = {k["kernel"]: k for k in ctx.kernel_times()}
        ctx.set_timing(0)
        assert all(kt[k]["launches"] == 1 for k in KERNELS), kt
        if rep:                                            # repetition 0 is the warm-up
            for k in KERNELS:
                per[k].append(kt[k]["total_ms"])
    floor_ms = 4.0 * B * H * W * (cin + cout) / HBM * 1e3
    row = {"cin": cin, "cout": cout, "streaming_floor_ms": round(floor_ms, 4)}
    for k in KERNELS:
        row[k] = stats(per[k])
        if k != "conv1x1_wgrad_reduce_kernel":
            row[k]["x_floor"] = round(row[k]["ms_median"] / floor_ms, 2)
    res["operator"].append(row)
    print(json.dumps(row), flush=True)
    for p in (x, g, gin):
        ctx.free(p)
    net.close()

block = synth.init_params(models.createResidual(64, 32, 64), 5)
block.training()
device.compile_models(synth.normal((2, 64, H, W), 1), block)
dm = device.DeviceModel(ctx, block)
n = B * 64 * H * W
x, g = ctx.malloc(4 * n), ctx.malloc(4 * n)
ctx.fill_normal(x, n, 2); ctx.fill_normal(g, n, 3)


def step():
    dm.zero_grads(); dm.forward(x, B); dm.backward(g, B, True)


step()                                                     # the warm-up, discarded
for i in range(REPS):
    ctx.event_record(2 * i); step(); ctx.event_record(2 * i + 1)
ctx.synchronize()
res["block"] = dict({"model": "createResidual(64, 32, 64)", "what": "zero_grads + forward + backward, training mode"},
                    **stats([ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS)]))
ctx.set_timing(2); step(); ctx.synchronize()
kt = [k for k in ctx.kernel_times() if k.get("launches")]
ctx.set_timing(0)
res["block"]["kernels"] = sorted(({"kernel": k["kernel"], "launches": k["launches"], "total_ms": round(k.get("total_ms", 0.0), 4)} for k in kt),
                                 key=lambda k: -k["total_ms"])[:12]
print(json.dumps(res["block"]), flush=True)
ctx.free(x); ctx.free(g); dm.close()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_residual.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
