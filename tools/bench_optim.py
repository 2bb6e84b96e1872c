#!/usr/bin/env python3
"""gr_optim_step (penalty + clamp + sgd | adagrad | adadelta | adamax | rmsprop, one fused launch each) against gr_adam_step
(penalty_clamp_adam_kernel, the yardstick) on one flat vector, event-timed on the context's stream: median [min, max] of 30 warmed-up launches
at the parameter counts of create_D2 and create_G3 for 3x64x64, and the bytes per second that makes with each method's own traffic (16 bytes an
entry for plain sgd, 24 for sgd with momentum, adagrad and rmsprop, 32 for adadelta, adamax and adam).  adam is timed first and again last, so
a drift of the clock over the run shows.  Then the number the device-resident path exists for: one GAN batch with --D_optmethod sgd
--G_optmethod sgd at batch 32, adversarial.DeviceGame against the --compat game (adversarial.train), at ganrev.train's default 1x32x32 and at
3x64x64.   python tools/bench_optim.py [out.json]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import adversarial, models, nn, synth
from ganrev.synth import synthetic_images

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
res = {"device": ctx.info(), "steps": [], "game": []}
WARM, REPS = 10, 30
PEN = dict(l1=0.0, l2=1e-4, clamp=1.0)
BYTES = {"adam": 32, "sgd": 16, "sgd-momentum": 24, "adagrad": 24, "adadelta": 32, "adamax": 32, "rmsprop": 24}
CONFIGS = {"sgd": ("sgd", {"learningRate": 0.02}), "sgd-momentum": ("sgd", {"learningRate": 0.02, "momentum": 0.5}), "adagrad": ("adagrad", {}),
           "adadelta": ("adadelta", {}), "adamax": ("adamax", {}), "rmsprop": ("rmsprop", {})}


def timed(fn):
    for _ in range(WARM):
        fn()
    for i in range(REPS):
        ctx.event_record(2 * i); fn(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    ms = sorted(ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS))
    return ms[REPS // 2], ms[0], ms[-1]


DIMS = (3, 64, 64)
for name, n in (("D2", models.create_D2(DIMS)._param_count()), ("G3", models.create_G3(DIMS, 100)._param_count())):
    lin = nn.Linear(n - 1, 1)                                  # a net whose flat vector has exactly n entries
    lin.forward(synth.normal((1, n - 1), 1))
    net = lin._net
    assert net.n_params == n
    net.set_params(synth.normal((n,), 2) * np.float32(0.05)); net.set_grads(synth.normal((n,), 3) * np.float32(0.7))
    rows = {}
    for label in ["adam"] + list(CONFIGS) + ["adam_again"]:
        net.optim_reset()
        if label.startswith("adam"):
            h = L.Hyper(**PEN)
            med, lo, hi = timed(lambda: net.adam_step(h, 2))
        else:
            cfg = L.OptimConfig(*CONFIGS[label], **PEN)
            med, lo, hi = timed(lambda: net.optim_step(cfg, 2))
        nbytes = BYTES[label.split("_")[0]] * n
        rows[label] = row = {"net": name, "params": n, "method": label, "bytes": nbytes, "ms_median": round(med, 5), "ms_min": round(lo, 5),
                             "ms_max": round(hi, 5), "GBps": round(nbytes / med / 1e6, 1)}
        res["steps"].append(row)
        print(f"{name} {n} {label}: {med * 1e3:.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}], {nbytes} B, {row['GBps']} GB/s", flush=True)
    adam_max = max(rows["adam"]["ms_max"], rows["adam_again"]["ms_max"])
    for label in CONFIGS:
        rows[label]["slower_than_adams_max"] = bool(rows[label]["bytes"] < rows["adam"]["bytes"] and rows[label]["ms_median"] > adam_max)
    del net, lin

B, STEPS, GWARM = 32, 20, 3
for dims in ((1, 32, 32), DIMS):
    def env_of():
        G, D = models.create_G(dims, 100, True, 2), models.create_D(dims, True, 1)
        return adversarial.make_env(G, D, dims, batchSize=B, N_epoch=STEPS, D_optmethod="sgd", G_optmethod="sgd")
    real = synthetic_images(STEPS * B // 2, dims, 7)
    env = env_of()
    game = adversarial.DeviceGame(env)
    for b in range(GWARM):
        game.batch(real[b * (B // 2):(b + 1) * (B // 2)])
    ctx.synchronize()
    t0 = time.perf_counter()
    for b in range(STEPS):
        game.batch(real[b * (B // 2):(b + 1) * (B // 2)])
    ctx.synchronize()
    dev_ms = (time.perf_counter() - t0) / STEPS * 1e3
    game.close()
    env = env_of()
    env.OPT.N_epoch = GWARM
    adversarial.train(env, real)
    env.OPT.N_epoch = STEPS
    ctx.synchronize()
    t0 = time.perf_counter()
    adversarial.train(env, real)
    ctx.synchronize()
    host_ms = (time.perf_counter() - t0) / STEPS * 1e3
    row = {"dims": list(dims), "batch": B, "D_optmethod": "sgd", "G_optmethod": "sgd", "batches_timed": STEPS, "device_game_ms_per_batch": round(dev_ms, 4),
           "compat_game_ms_per_batch": round(host_ms, 4), "compat_over_device": round(host_ms / dev_ms, 2)}
    res["game"].append(row)
    print(f"GAN batch {dims} batch {B}, sgd / sgd: device game {dev_ms:.3f} ms, --compat game {host_ms:.3f} ms, ratio {host_ms / dev_ms:.2f}", flush=True)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_optim.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
