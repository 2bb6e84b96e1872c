#!/usr/bin/env python3
"""What a VAE step costs next to the autoencoder step it grew from: train_vae.DeviceLoop.batch against pretrain_g.DeviceLoop.batch at the same
shapes (1x32x32 and 3x64x64, batch 128, noiseDim 100), same process, same box; and the parts the VAE step adds, each timed alone: the two
sampling launches (gr_vae_sample_dev with its KL mean, gr_vae_sample_backward_dev), the eps fill, the decoder's backward with and without its
input gradient (the difference is the input-gradient GEMM of its first nn.Linear), Adam and zero_grads on two nets against one.  Event-timed on
the context's stream (the events see the host work between two launches too, as wall time), median [min, max] of 30 after one discarded
warm-up; the autoencoder step is timed first and again last, so a drift over the run shows.   python tools/bench_vae.py [out.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import ganrev._lib as L
from ganrev import pretrain_g, train_vae
from ganrev.synth import synthetic_images

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
REPS, B, ND = 30, 128, 100
res = {"device": ctx.info(), "reps": REPS, "batch": B, "noiseDim": ND, "conv_mode": "f16x3", "cases": []}


def timed(fn):
    fn()                                                       # the warm-up, discarded
    for i in range(REPS):
        ctx.event_record(2 * i); fn(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    ms = sorted(ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS))
    return {"ms_median": round(ms[REPS // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


for dims in ((1, 32, 32), (3, 64, 64)):
    hyper = L.Hyper(l1=0.0, l2=0.0, clamp=5.0)
    images = synthetic_images(B, dims, 7)
    ae = pretrain_g.build(dims, ND, 1)
    ae._ctx = ctx
    ae_loop = pretrain_g.DeviceLoop(ae, dims, B, hyper)
    ae_loop.load(images)
    enc, dec = train_vae.build(dims, ND, 1)
    enc._ctx = dec._ctx = ctx
    loop = train_vae.DeviceLoop(enc, dec, dims, ND, B, hyper, "mse", 1, None, 0)
    loop.load(images)
    row = {"dims": list(dims)}
    row["autoencoder_step"] = timed(lambda: ae_loop.batch(0))
    row["vae_step"] = timed(lambda: loop.batch(0))
    loop.forward(0)                                            # the state the parts below read: h, eps, z, the criterion's gradient
    loop.backward()

    def sampling():
        ctx.vae_sample_dev(loop.h, loop.eps, B, ND, loop.z, None, loop.kl)
        ctx.vae_sample_backward_dev(loop.h, loop.eps, loop.z, B, ND, loop.kl_weight, loop.gh)      # (z stands in for gz: the same shape)
    row["sampling_launches"] = timed(sampling)
    row["eps_fill"] = timed(lambda: ctx.fill_normal(loop.eps, B * ND, 5))
    row["decoder_backward_with_input_gradient"] = timed(lambda: loop.dec.backward(loop.grad, B, True))
    row["decoder_backward_without"] = timed(lambda: loop.dec.backward(loop.grad, B, False))
    row["adam_two_nets"] = timed(loop.step)
    row["adam_one_net"] = timed(lambda: ae_loop.net.adam_step(hyper, ae_loop.t))

    def zero_two():
        loop.enc.zero_grads(); loop.dec.zero_grads()
    row["zero_grads_two_nets"] = timed(zero_two)
    row["zero_grads_one_net"] = timed(ae_loop.net.zero_grads)
    row["autoencoder_step_again"] = timed(lambda: ae_loop.batch(0))
    m = lambda k: row[k]["ms_median"]
    row["vae_minus_autoencoder_ms"] = round(m("vae_step") - m("autoencoder_step"), 4)
    row["sum_of_parts_ms"] = round(m("sampling_launches") + m("eps_fill") + m("decoder_backward_with_input_gradient") - m("decoder_backward_without")
                                   + m("adam_two_nets") - m("adam_one_net") + m("zero_grads_two_nets") - m("zero_grads_one_net"), 4)
    res["cases"].append(row)
    print(json.dumps(row), flush=True)
    loop.close(); ae_loop.close()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_vae.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
