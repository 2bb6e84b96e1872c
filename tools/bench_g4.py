#!/usr/bin/env python3
"""models.create_G4((1, 32, 32), 100) as a bundle (one grouped gr_net, nn.bundle_plan) and on the parts route (`concat.bundle = False`: 32
branch nets and a tail net inside device.DeviceModel), with models.create_G3 beside them, in one process, f16x3 arithmetic:
  * the evaluate() forward at batch 256 and 512;
  * the adversarial.DeviceGame step against models.create_D2 at batch 32 and 256;
  * the kernels of csrc/group.hip in a training-mode forward + backward of the bundle at batch 256, each under its own pair of events
    (gr_set_timing 2), next to its streaming floor: the bytes it must move at the 8 TB/s HBM rate DESIGN.md uses - with the tuning key
    group_mfma_min_tiles at 2^30, so the grouped convolution runs on the fp32 kernels;
  * the three launches of csrc/groupmfma.hip that replace them (key at 1), f16x3 and bf16x6, and both families again at batch 16: the
    crossover the key's default is set by.
The forward and game rows run at the library's default key (512 tiles: the MFMA launches from batch 16 on).
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
KEY, NEVER = "group_mfma_min_tiles", 1 << 30
G = make_g("create_G4 bundle")
G.training()
G.forward(synth.normal((2, ND), 1))
net = G._net
nb, K, M, P = 32, 16, 4096, 16                             # branches, inputs / outputs per group of the grouped Linear, planes per group


def floors(B):
    """bytes each kernel must move (fp32): inputs read once, outputs written once"""
    fl = 4.0 * B * nb
    conv = fl * P * (256 + 1024)
    return {
        "grouplinear_forward_kernel": fl * (K + M) + 4.0 * nb * M * (K + 1),
        "grouplinear_dgrad_kernel": fl * (K + M) + 4.0 * nb * M * K,
        "grouplinear_wgrad_kernel": fl * (K + M) + 8.0 * nb * M * K,
        "groupconv3_forward_kernel": conv, "groupconv3_dgrad_kernel": conv, "groupconv3_wgrad_kernel": conv,
        "groupconv3_mfma_forward_kernel": conv, "groupconv3_mfma_dgrad_kernel": conv, "groupconv3_mfma_wgrad_kernel": conv,
        "prelu_multi_forward_kernel": 2 * fl * (K + M + P * 1024),          # the three nn.PReLU layers of the bundle together
        "prelu_multi_backward_kernel": 3 * fl * (K + M + P * 1024),
        "prelu_multi_grad_kernel": 2 * fl * (K + M + P * 1024),
    }


def kernel_rows(B, mode, key, only=None):
    """per-step totals of every FLOORS kernel the step launches (only: a name filter), the key and the arithmetic as given"""
    noise, gout = ctx.malloc(4 * B * ND), ctx.malloc(4 * B * 1024)
    ctx.fill_normal(noise, B * ND, 3); ctx.fill_normal(gout, B * 1024, 4)
    ctx.set_conv_mode(mode); ctx.set_tuning(KEY, key)
    fl = floors(B)
    per = {}
    try:
        for rep in range(REPS + 1):
            ctx.set_timing(2)
            net.zero_grads(); net.forward_dev(noise, B); net.backward_dev(noise, gout, B, None)
            ctx.synchronize()
            kt = {k["kernel"]: k for k in ctx.kernel_times()}
            ctx.set_timing(0)
            if rep:
                for k in fl:
                    if k in kt and (only is None or only in k):
                        per.setdefault(k, []).append(kt[k]["total_ms"])
    finally:
        ctx.set_timing(0); ctx.set_conv_mode("f16x3"); ctx.set_tuning(KEY, 512)
        ctx.free(noise); ctx.free(gout)
    rows = []
    for k, ms in per.items():
        floor_ms = fl[k] / HBM * 1e3
        row = dict({"kernel": k, "batch": B, "arithmetic": mode if "mfma" in k else "fp32", "launches_per_step": kt[k]["launches"],
                    "streaming_floor_ms": round(floor_ms, 4)}, **stats(ms))
        row["x_floor"] = round(row["ms_median"] / floor_ms, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


res["kernels"] = {"batch": 256, "what": "training-mode forward + backward of the bundle; per-step totals of each kernel; group_mfma_min_tiles at 2^30 (the grouped convolution on the fp32 kernels)",
                  "rows": kernel_rows(256, "f16x3", NEVER)}
res["kernels_mfma"] = {"what": "the same step with group_mfma_min_tiles at 1: the grouped convolution's three launches on the MFMA kernels, and the fp32 ones at batch 16 beside them",
                       "rows": kernel_rows(256, "f16x3", 1, "groupconv3") + kernel_rows(256, "bf16x6", 1, "groupconv3")
                       + kernel_rows(16, "f16x3", NEVER, "groupconv3") + kernel_rows(16, "f16x3", 1, "groupconv3") + kernel_rows(16, "bf16x6", 1, "groupconv3")}

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_g4.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
