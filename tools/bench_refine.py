#!/usr/bin/env python3
"""One refinement step of ganrev.refine.refineNoise on models.create_G3, batch 256, f16x3 arithmetic, at 1 x 32 x 32 / noiseDim 32 and at
3 x 64 x 64 / noiseDim 100, in one process:
  * the step (forward with the input-gradient flag on, gr_mse_rows_dev, gr_net_backward_input_dev, gr_adam_rows_step_dev) and each of its four parts;
  * beside them the evaluate() forward with the flag off (fused epilogues, operand-ready hand-overs: what the flag gives up) and the existing full
    backward, gr_net_backward_dev after a training-mode forward of the same net (every weight, bias and BatchNorm gradient formed).
Event-timed on the context's stream, median [min, max] of 30 after one discarded warm-up; a backward is repeated after ONE forward (it reads the
forward's state and leaves it as it was).
   python tools/bench_refine.py [out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import device, models, synth

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
REPS, B = 30, 256
res = {"device": ctx.info(), "reps": REPS, "batch": B, "conv_mode": "f16x3", "rows": []}


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def timed(step):
    step()                                                 # the warm-up, discarded
    for i in range(REPS):
        ctx.event_record(2 * i); step(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    return stats([ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS)])


for dims, nd in (((1, 32, 32), 32), ((3, 64, 64), 100)):
    G = synth.init_params(models.create_G3(dims, nd, seed=1), 2)
    G.evaluate()
    G.forward(synth.normal((2, nd), 1))                    # compile
    dm = device.DeviceModel(ctx, G)
    net, n = dm.nets[0], int(np.prod(dims))
    z, x, g, gz = ctx.malloc(4 * B * nd), ctx.malloc(4 * B * n), ctx.malloc(4 * B * n), ctx.malloc(4 * B * nd)
    m, v, bz = (ctx.upload(np.zeros(B * nd, np.float32)) for _ in range(3))
    loss, best = ctx.malloc(4 * B), ctx.upload(np.full(B, np.inf, np.float32))
    ctx.fill_normal(z, B * nd, 3); ctx.fill_uniform(x, B * n, 4, 0.0, 1.0)
    hyper = L.AdamHyper(lr=1e-6)                           # (z barely moves: every repetition times the same work)
    rows = {}
    dm.set_training(False); dm.set_input_grad(False)
    rows["evaluate() forward, flag off"] = timed(lambda: dm.forward(z, B))
    dm.set_input_grad(True)
    out = dm.forward(z, B)

    def step():
        o = dm.forward(z, B)
        ctx.mse_rows_dev(o, x, B, n, loss, g)
        ctx.adam_rows_step_dev(z, dm.backward(g, B, True, params=False), m, v, B, nd, hyper, 1, loss, best, bz)
    rows["refinement step"] = timed(step)
    rows["forward, flag on"] = timed(lambda: dm.forward(z, B))
    rows["criterion (gr_mse_rows_dev)"] = timed(lambda: ctx.mse_rows_dev(out, x, B, n, loss, g))
    rows["input-only backward (gr_net_backward_input_dev)"] = timed(lambda: net.backward_input_dev(z, g, B, gz))
    rows["Adam (gr_adam_rows_step_dev)"] = timed(lambda: ctx.adam_rows_step_dev(z, gz, m, v, B, nd, hyper, 1, loss, best, bz))
    dm.set_input_grad(False); dm.set_training(True)
    rows["training-mode forward"] = timed(lambda: dm.forward(z, B))
    net.zero_grads()
    rows["full backward (gr_net_backward_dev, training mode)"] = timed(lambda: net.backward_dev(z, g, B, gz))
    dm.set_training(False)
    G.push_bn_running()
    a, b = rows["input-only backward (gr_net_backward_input_dev)"]["ms_median"], rows["full backward (gr_net_backward_dev, training mode)"]["ms_median"]
    for what, st in rows.items():
        row = dict({"model": "create_G3", "dims": list(dims), "noiseDim": nd, "what": what}, **st)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    ratio = {"model": "create_G3", "dims": list(dims), "noiseDim": nd, "input_only_over_full_backward": round(a / b, 4)}
    res["rows"].append(ratio)
    print(json.dumps(ratio), flush=True)
    for p in (z, x, g, gz, m, v, bz, loss, best):
        ctx.free(p)
    dm.close()

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_refine.json")
json.dump(res, open(out, "w"), indent=1)
print("wrote", out)
