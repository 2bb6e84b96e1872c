#!/usr/bin/env python3
"""models.create_G4((1, 32, 32), 100) as a bundle (one grouped gr_net, nn.bundle_plan) and on the parts route (`concat.bundle = False`: 32
branch nets and a tail net inside device.DeviceModel), with models.create_G3 beside them, in one process, f16x3 arithmetic:
  * the evaluate() forward at batch 256 and 512;
  * the adversarial.DeviceGame step against models.create_D2 at batch 32 and 256;
  * the kernels of csrc/group.hip in a training-mode forward + backward of the bundle at batch 256, each under its own pair of events
    (gr_set_timing 2), next to its streaming floor: the bytes it must move at the 8 TB/s HBM rate DESIGN.md uses.
Event-timed on the context's stream, median [min, max] of 30 after one discarded warm-up.
   python tools/bench_g4.py [out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import adversarial, device, models, synth

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
REPS, DIMS, ND, HBM = 30, (1, 32, 32), 100, 8.0e12
res = {"device": ctx.info(), "reps": REPS, "dims": list(DIMS), "noiseDim": ND, "hbm_bytes_per_s": HBM, "forward": [], "game": [], "kernels": None}


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def timed(step):
    step()                                                 # the warm-up, discarded
    for i in range(REPS):
        ctx.event_record(2 * i); step(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    return stats([ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS)])


def make_g(route):
    if route == "create_G3":
        return synth.init_params(models.create_G3(DIMS, ND, seed=1), 2)
    G = synth.init_params(models.create_G4(DIMS, ND, seed=1), 2)
    if route == "create_G4 parts":
        G.modules[1].bundle = False
    return G


ROUTES = ("create_G4 bundle", "create_G4 parts", "create_G3")

for B in (256, 512):
    noise = ctx.malloc(4 * B * ND)
    ctx.fill_normal(noise, B * ND, 3)
    for route in ROUTES:
        G = make_g(route)
        G.evaluate()
        G.forward(synth.normal((2, ND), 1))                # compile
        dm = device.DeviceModel(ctx, G)
        dm.set_training(False)
        row = dict({"model": route, "batch": B, "nets": len(dm.nets), "what": "evaluate() forward"}, **timed(lambda: dm.forward(noise, B)))
        res["forward"].append(row)
        print(json.dumps(row), flush=True)
        dm.close()
    ctx.free(noise)

for B in (32, 256):
    real = synth.uniform((B // 2,) + DIMS, 5, 0, 1)
    for route in ROUTES:
        G, D = make_g(route), models.create_D2(DIMS, True, 4)
        env = adversarial.make_env(G, D, DIMS, batchSize=B, noiseDim=ND, N_epoch=1)
        game = adversarial.DeviceGame(env)
        row = dict({"model": route, "batch": B, "nets_G": len(game.gg.nets), "what": "DeviceGame.batch against create_D2 (one D and one G iteration, the upload of the real half included)"},
                   **timed(lambda: game.batch(real)))
        res["game"].append(row)
        print(json.dumps(row), flush=True)
        game.close()

# the grouped kernels inside the bundle's training step
B = 256
G = make_g("create_G4 bundle")
G.training()
G.forward(synth.normal((2, ND), 1))
net = G._net
noise, gout = ctx.malloc(4 * B * ND), ctx.malloc(4 * B * 1024)
ctx.fill_normal(noise, B * ND, 3); ctx.fill_normal(gout, B * 1024, 4)
nb, K, M, P = 32, 16, 4096, 16                             # branches, inputs / outputs per group of the grouped Linear, planes per group
fl = 4.0 * B * nb
FLOORS = {   # bytes each kernel must move (fp32): inputs read once, outputs written once
    "grouplinear_forward_kernel": fl * (K + M) + 4.0 * nb * M * (K + 1),
    "grouplinear_dgrad_kernel": fl * (K + M) + 4.0 * nb * M * K,
    "grouplinear_wgrad_kernel": fl * (K + M) + 8.0 * nb * M * K,
    "groupconv3_forward_kernel": fl * P * (256 + 1024),
    "groupconv3_dgrad_kernel": fl * P * (256 + 1024),
    "groupconv3_wgrad_kernel": fl * P * (256 + 1024),
    "prelu_multi_forward_kernel": 2 * fl * (K + M + P * 1024),          # the three nn.PReLU layers of the bundle together
    "prelu_multi_backward_kernel": 3 * fl * (K + M + P * 1024),
    "prelu_multi_grad_kernel": 2 * fl * (K + M + P * 1024),
}
per = {k: [] for k in FLOORS}
for rep in range(REPS + 1):
    ctx.set_timing(2)
    net.zero_grads(); net.forward_dev(noise, B); net.backward_dev(noise, gout, B, None)
    ctx.synchronize()
    kt = {k["kernel"]: k for k in ctx.kernel_times()}
    ctx.set_timing(0)
    if rep:
        for k in FLOORS:
            per[k].append(kt[k]["total_ms"])
rows = []
for k, nbytes in FLOORS.items():
    floor_ms = nbytes / HBM * 1e3
    row = dict({"kernel": k, "launches_per_step": kt[k]["launches"], "streaming_floor_ms": round(floor_ms, 4)}, **stats(per[k]))
    row["x_floor"] = round(row["ms_median"] / floor_ms, 2)
    rows.append(row)
    print(json.dumps(row), flush=True)
res["kernels"] = {"batch": B, "what": "training-mode forward + backward of the bundle; per-step totals of each kernel", "rows": rows}
ctx.free(noise); ctx.free(gout)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_g4.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
