"""gpu: ganrev.pretrain_with_previous_net (pretrain_with_previous_net.lua:92-266) - one batch of the device-resident loop against the
oracle, the fast loop against --compat, the script end to end, and the yuv / hsl choices of ganrev.pretrain_g.

The oracle batch is built the way test_gpu_parity.py::test_adversarial_step_vs_oracle builds its case: helpers.OracleGraph for the two
D nets, the plain oracle for the two G nets, tests/colorspace_oracle.py's fp32 twin for the two conversions in between; dropout masks
injected, pool argmax and PReLU / ReLU kinks adopted from the device.  Bars: helpers.TOL, assert_close, assert_grads_close with the
floors that test uses for fevalD (1e-3) and for G's gradient (1e-6); parameters after Adam where |g| > 1e-4.

(y, rgb), (rgb, yuv) and (yuv, y) are linear conversions with coefficients of at most 2.04: the 3e-6 device error of G_PREV's images
reaches D's input and the MSE target at most 3 x larger, inside TOL.  rgb -> hsl divides by d = max - min and wraps the hue: on
device-computed images it is ill-conditioned against an independently computed oracle - a property of the reference algorithm, like
the pool near-ties.  The (hsl, rgb) and (rgb, hsl) cases therefore feed the oracle the DEVICE's converted tensors and compare everything
behind them to the same bars; the conversions themselves are held bit-exact by tests/test_gpu_colorspace.py (and, here, on the real
half of D's input, which is no network output).
"""
import hashlib
import os

import numpy as np
import pytest

import colorspace_oracle as co
from helpers import TOL, OracleGraph, adopt_device_argmax, adopt_device_kinks, assert_close, assert_grads_close, dropout_modules, maxdiff

pytestmark = pytest.mark.gpu

H = W = 16
B = 8


def _opts(prev, cur, pnd, nd, extra=()):
    from ganrev import pretrain_with_previous_net as P
    OPT = P.parse(["--batchSize", str(B), "--height", str(H), "--width", str(W), "--colorSpace", cur, "--noiseDim", str(nd), "--quiet"] + list(extra))
    return OPT, (pnd, "normal", prev, H, W)


def _inject(chunk, onet, seed):
    """the same keep flags into the oracle net and straight into the compiled net (the *_dev calls do not pass through Module.forward)"""
    from ganrev import synth
    for m in dropout_modules(chunk):
        li = onet.layer_index[id(m)]
        keep = synth.bernoulli_keep((onet.mask_size(li, B),), seed * 131 + li, m.p)
        onet.set_mask(li, keep)
        chunk._net.set_mask(chunk._leaf_layer(m), keep)


CASES = [("y", "rgb", 32, 100), ("rgb", "yuv", 100, 100), ("yuv", "y", 100, 32), ("hsl", "rgb", 32, 100), ("rgb", "hsl", 100, 32)]


@pytest.mark.parametrize("prev,cur,pnd,nd", CASES, ids=lambda v: str(v))
def test_one_batch_vs_oracle(oracle, ctx, conv_mode, prev, cur, pnd, nd):
    from ganrev import models, synth
    from ganrev import pretrain_with_previous_net as P
    OPT, po = _opts(prev, cur, pnd, nd)
    pdims, dims = P.image_dims(prev, H, W), P.image_dims(cur, H, W)
    G_PREV = models.create_G(pdims, pnd, seed=1); synth.init_params(G_PREV, 2)
    D_PREV = models.create_D2(pdims, seed=2); synth.init_params(D_PREV, 3)
    G = models.create_G(dims, nd, seed=3); synth.init_params(G, 4)
    D = models.create_D2(dims, seed=4); synth.init_params(D, 5)
    oGp = oracle.from_model(G_PREV, (pnd, 1, 1)); oGp.set_training(False)
    oG = oracle.from_model(G, (nd, 1, 1)); oG.set_training(True)
    ogp = OracleGraph(oracle, D_PREV, pdims); ogp.set_training(False)
    og = OracleGraph(oracle, D, dims); og.set_training(True)
    s = P.setup(OPT, G_PREV, D_PREV, po, G=G, D=D)
    loop = P.DeviceDistill(s)
    try:
        theta_g = oG.params.copy()
        theta_d = np.concatenate([o.params for _, o in og.pairs])
        assert np.array_equal(theta_g, loop.gnet.get_params())
        assert np.array_equal(theta_d, np.concatenate([n.get_params() for n in loop.dg.nets]))
        half = B // 2
        prev_noise, noise = synth.normal((B, pnd), 5), synth.normal((B, nd), 6)
        real = synth.uniform((half, 3, H, W), 7, 0, 1)
        shared = min(pnd, nd)
        noise_ref = noise.copy(); noise_ref[:, :shared] = prev_noise[:, :shared]            # :155-159, in both directions over the cases
        _inject(G, oG, 21)
        for chunk, onet in og.pairs:
            _inject(chunk, onet, 21)
        loop.forward(real, prev_noise, noise)
        dl = ctx.download
        assert np.array_equal(dl(loop.noise, (B, nd)), noise_ref), "the shared noise columns"
        assert np.array_equal(dl(loop.prev_noise, (B, pnd)), prev_noise)
        hsl = "hsl" in (prev, cur)

        # ---- imagesByGprev after the conversion (:166-167)
        raw = oGp.forward(prev_noise)
        dev_raw = dl(loop.gprev.lib.gr_net_output_dev(loop.gprev.h), (B,) + pdims)
        assert_close(dev_raw, raw, TOL, "G_PREV(prevNoise)")
        dev_imgs_prev = dl(loop.images_by_gprev, (B,) + dims)
        assert np.array_equal(dev_imgs_prev.view(np.uint32), co.switch(dev_raw, prev, cur).view(np.uint32)), "the conversion of the device's own images"
        if hsl:
            imgs_prev = dev_imgs_prev                # the oracle continues from the device's converted tensor (module docstring)
        else:
            imgs_prev = co.switch(raw, prev, cur)
            assert_close(dev_imgs_prev, imgs_prev, TOL, "imagesByGprev in the new colour space")

        # ---- imagesDinput (:170-180): half real (rgb -> cur, bit-exact: no network in front), the FIRST half of imagesByGprev
        dev_dinput = dl(loop.d_input, (B,) + dims)
        assert np.array_equal(dev_dinput[:half].view(np.uint32), co.from_rgb(real, cur).view(np.uint32)), "the real half of D's input"
        assert np.array_equal(dev_dinput[half:], dev_imgs_prev[:half]), "the generated half of D's input"
        dinput = np.concatenate([co.from_rgb(real, cur), imgs_prev[:half]]).astype(np.float32)
        assert_close(dev_dinput, dinput, TOL, "imagesDinput")

        # ---- predsByDprev (:182)
        dev_dinput_prev = dl(loop.d_input_prev, (B,) + pdims)
        assert np.array_equal(dev_dinput_prev.view(np.uint32), co.switch(dev_dinput, cur, prev).view(np.uint32)), "D_PREV's input"
        dinput_prev = dev_dinput_prev if hsl else co.switch(dinput, cur, prev)
        if not hsl:
            assert_close(dev_dinput_prev, dinput_prev, TOL * 3, "imagesDinput in the previous colour space (coefficients up to 2.04)")
        preds_prev = ogp.forward(dinput_prev)
        dev_preds_prev = dl(loop.preds_by_dprev, (B, 1))
        assert_close(dev_preds_prev, preds_prev, TOL, "predsByDprev")

        # ---- predsByD (:183) and imagesByG (:168), then the device's pool argmax and kinks onto the oracle
        ref_out = og.forward(dinput)
        dev_out = dl(loop.preds_by_d, (B, 1))
        assert_close(dev_out, ref_out, TOL, "predsByD")
        for chunk, onet in og.pairs:
            adopt_device_argmax(chunk, onet, B, 16)
        ref_out = og.forward(dinput)
        assert_close(dev_out, ref_out, TOL, "predsByD vs the argmax-forced oracle")
        for chunk, onet in og.pairs:
            adopt_device_kinks(chunk, onet, B, 16)
        rimg = oG.forward(noise_ref)
        assert_close(dl(loop.images_by_g, (B,) + dims), rimg, TOL, "imagesByG")
        adopt_device_kinks(G, oG, B, 16)

        # ---- fevalG / fevalD up to the backward (:185-194, :213-222)
        loop.backward()
        rd = lambda p: float(dl(p, (1,), np.float64)[0])
        rf_g, rdf_g = oracle.mse(rimg, imgs_prev)
        oG.zero_grads(); oG.backward(noise_ref, rdf_g.reshape(rimg.shape))
        rg_g = oG.grads.copy()
        rf_d, rdf_d = oracle.bce(ref_out.reshape(-1), preds_prev.reshape(-1))
        og.zero_grads(); og.backward(dinput, rdf_d.reshape(ref_out.shape))
        rg_d = og.grads.copy()
        f_g, f_d = rd(loop.loss_g), rd(loop.loss_d)
        print(f"[distill {prev}->{cur} {conv_mode}] loss G {f_g:.6f} (oracle {rf_g:.6f}), loss D {f_d:.6f} (oracle {rf_d:.6f})")
        assert abs(f_g - rf_g) <= 1e-5 * max(1.0, abs(rf_g)), f"loss G {f_g} vs {rf_g}"
        assert abs(f_d - rf_d) <= 1e-5 * max(1.0, abs(rf_d)), f"loss D {f_d} vs {rf_d}"
        g_g = loop.gnet.get_grads()
        g_d = np.concatenate([n.get_grads() for n in loop.dg.nets])
        assert_grads_close(G, g_g, rg_g, 1e-4, 1e-6, "G before penalty + clamp")
        assert_grads_close(D, g_d, rg_d, 1e-4, 1e-3, "D before penalty + clamp")

        # ---- penalty + clamp (:196-208, :224-236) and optim.adam (:241-242)
        loop.step()
        for name, model, nets, theta, rg, l1w, l2w, cl, floor in (("G", G, [loop.gnet], theta_g, rg_g, OPT.G_L1, OPT.G_L2, OPT.G_clamp, 1e-6),
                                                                  ("D", D, loop.dg.nets, theta_d, rg_d, OPT.D_L1, OPT.D_L2, OPT.D_clamp, 1e-3)):
            rtheta, rgc = theta.copy(), rg.copy()
            m, v = np.zeros_like(rtheta), np.zeros_like(rtheta)
            oracle.penalty_clamp_adam(rtheta, rgc, m, v, oracle.GoHyper(l1=l1w, l2=l2w, clamp=cl), 1)
            got_g = np.concatenate([n.get_grads() for n in nets])
            got_theta = np.concatenate([n.get_params() for n in nets])
            assert_grads_close(model, got_g, rgc, 1e-4, floor, f"{name} after penalty + clamp")
            well = np.abs(rgc) > 1e-4                 # entries whose Adam step is well-conditioned
            assert well.any()
            assert_close(got_theta[well], rtheta[well], TOL, f"{name}'s parameters after Adam")
            assert maxdiff(got_theta, rtheta) <= 2.1e-3     # nothing moved by more than one lr-sized Adam step either way
    finally:
        loop.close()


def _previous_checkpoint(tmp_path, colorSpace="rgb", nd=16):
    from ganrev import train
    d = tmp_path / "prev"
    r = train.main(["--epochs", "1", "--N_epoch", "1", "--batchSize", "4", "--noiseDim", str(nd), "--height", str(H), "--width", str(W),
                    "--colorSpace", colorSpace, "--save", str(d), "--quiet"])
    return r["path"]


def _flat(model):
    return model._flat_host() if model._flat is None else model._flat[0].copy()


def _bn(model):
    return [(m.running_mean.copy(), m.running_var.copy()) for m in model.leaves() if hasattr(m, "running_mean")]


def test_fast_loop_matches_compat(ctx, conv_mode, tmp_path):
    """Both loops from the same seed: the same Philox noise and dropout streams, the same kernels.  f32 / bf16x6: three batches, the
    parameters, Adam's moments and the BatchNorm running statistics bit-identical.  f16x3: the host entry points of --compat are
    range-guarded and keep fp32 copies of every tensor, so they select other kernels than the device loop - last-bit differences,
    which Adam's normalised first step turns into +-lr where a gradient is within rounding of zero: the statement and the bars of
    tests/test_gpu_avgpool.py::test_pretrain_fast_matches_compat, which are bars for ONE Adam step - so one batch there."""
    from ganrev import pretrain_with_previous_net as P
    from helpers import param_segments
    net = _previous_checkpoint(tmp_path, "rgb", 16)
    nb = 1 if conv_mode == "f16x3" else 3
    args = ["--network", net, "--N_batches", str(nb), "--batchSize", str(B), "--noiseDim", "8", "--colorSpace", "yuv", "--height", str(H),
            "--width", str(W), "--saveFreq", "100", "--quiet", "--conv-mode", conv_mode]
    fast = P.main(args + ["--save", str(tmp_path / "fast")])
    fast_adam = {"G": fast["G"]._net.adam_state(), "D": [c._net.adam_state() for c, _, _ in fast["D"]._param_chunks()]}
    compat = P.main(args + ["--save", str(tmp_path / "compat"), "--compat"])
    st = compat["state"].OPTSTATE["adam"]
    for k in (0, 1):
        assert abs(fast["last_losses"][k] - compat["last_losses"][k]) <= 1e-5 * max(1.0, abs(compat["last_losses"][k])), (fast["last_losses"], compat["last_losses"])
    for name in ("G", "D"):
        pf, pc = _flat(fast[name]).astype(np.float64), _flat(compat[name]).astype(np.float64)
        d = np.abs(pf - pc)
        print(f"[distill fast vs compat] {conv_mode} {name}: max |dtheta| {d.max():.3e} after {nb} batch(es)")
        if conv_mode != "f16x3":
            assert d.max() == 0, f"{name}: parameters"
            fm = fast_adam[name] if name == "G" else tuple(np.concatenate([a[i] for a in fast_adam["D"]]) for i in (0, 1))
            assert np.array_equal(fm[0], st[name]["m"]) and np.array_equal(fm[1], st[name]["v"]), f"{name}: Adam state"
            for (am, av), (bm, bv) in zip(_bn(fast[name]), _bn(compat[name])):
                assert np.array_equal(am, bm) and np.array_equal(av, bv), f"{name}: BatchNorm running statistics"
            continue
        model = compat[name]
        leaves = model.leaves()
        residue = np.zeros(d.size, bool)
        for mod, nm, lo, hi in param_segments(model):
            i = leaves.index(mod)
            if nm == "bias" and i + 1 < len(leaves) and leaves[i + 1].typename.endswith("BatchNormalization") and not mod.typename.endswith("BatchNormalization"):
                residue[lo:hi] = True
        assert d.max() <= 2.1e-3, d.max()
        r = d[~residue]
        assert np.median(r) <= 1e-7 and (r > 1e-5).mean() <= 1e-2, (np.median(r), (r > 1e-5).mean())


def test_script_end_to_end(ctx, tmp_path):
    import ganrev._lib as L
    from ganrev import pretrain_with_previous_net as P
    from ganrev import synth, t7
    net = _previous_checkpoint(tmp_path, "gray", 16)                          # ganrev.train's name for one channel: read as "y"
    assert t7.load_checkpoint(net)["opt"]["colorSpace"] == "gray"
    np.save(str(tmp_path / "real.npy"), synth.uniform((6, 3, H, W), 3, 0, 1))
    common = ["--network", net, "--height", str(H), "--width", str(W), "--quiet"]
    r = P.main(common + ["--N_batches", "2", "--batchSize", "4", "--noiseDim", "8", "--colorSpace", "rgb", "--save", str(tmp_path / "out"),
                         "--saveFreq", "1", "--data", str(tmp_path / "real.npy")])
    path = os.path.join(str(tmp_path / "out"), "pretrained_3x16x16_nd8.net")
    assert r["path"] == path and os.path.isfile(path)
    assert r["state"].prev == (16, "normal", "y", H, W)
    assert all(np.isfinite(v) for v in r["last_losses"])
    ck = t7.load_checkpoint(path)
    assert "_unconverted" not in ck and {"G", "D", "opt"} <= set(ck)
    assert ck["opt"]["colorSpace"] == "rgb" and int(ck["opt"]["noiseDim"]) == 8
    G = ck["G"].evaluate()
    assert G.forward(synth.normal((2, 8), 1)).shape == (2, 3, H, W)
    assert np.array_equal(G._flat_host(), _flat(r["G"]))
    assert ck["D"].evaluate().forward(synth.uniform((2, 3, H, W), 2, 0, 1)).shape == (2, 1)
    with pytest.raises(L.GanrevError, match="even"):
        P.main(common + ["--N_batches", "1", "--batchSize", "5", "--save", str(tmp_path / "odd")])
    with pytest.raises(L.GanrevError, match="16 x 16"):
        P.main(["--network", net, "--height", "32", "--width", str(W), "--quiet", "--N_batches", "1", "--batchSize", "4", "--save", str(tmp_path / "h")])
    # the new noise dimension may also be LARGER than the old one, and the colour space may change on the way: one hsl batch, compat too
    for extra in ([], ["--compat"]):
        r = P.main(common + ["--N_batches", "1", "--batchSize", "4", "--noiseDim", "24", "--colorSpace", "hsl", "--save", str(tmp_path / "hsl")] + extra)
        assert os.path.basename(r["path"]) == "pretrained_3x16x16_nd24.net" and all(np.isfinite(v) for v in r["last_losses"])


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrain_g_rgb_checkpoint.sha256")
RGB_ARGS = ["--epochs", "1", "--N_epoch", "2", "--batchSize", "4", "--noiseDim", "16", "--colorSpace", "rgb", "--height", "16", "--width", "16",
            "--saveFreq", "1", "--quiet", "--conv-mode", "f32"]


def test_pretrain_g_accepts_yuv_and_leaves_rgb_alone(ctx, tmp_path, monkeypatch):
    """--colorSpace yuv on rgb data runs (fast and --compat see the same converted images) and saves opt.colorSpace = "yuv"; with rgb
    the checkpoint is byte-identical to the one the commit before this feature wrote for the same arguments (its SHA-256 is the
    recorded result under tests/golden/)."""
    from ganrev import pretrain_g, synth, t7
    rgb = synth.uniform((8, 3, H, W), 9, 0, 1)
    np.save(str(tmp_path / "rgb.npy"), rgb)
    args = ["--epochs", "1", "--N_epoch", "2", "--batchSize", "4", "--noiseDim", "16", "--height", str(H), "--width", str(W), "--saveFreq", "1",
            "--quiet", "--data", str(tmp_path / "rgb.npy"), "--conv-mode", "f32"]
    res = {}
    for cs in ("yuv", "hsl", "y"):
        for k in ("fast", "compat"):
            r = pretrain_g.main(args + ["--colorSpace", cs, "--save", str(tmp_path / (cs + k))] + (["--compat"] if k == "compat" else []))
            ck = t7.load_checkpoint(r["path"])
            assert ck["opt"]["colorSpace"] == cs and np.isfinite(r["last_loss"])
            assert os.path.basename(r["path"]) == "g_pretrained_%dx16x16_nd16.net" % (1 if cs == "y" else 3)
            res[cs, k] = r
        a, b = res[cs, "fast"], res[cs, "compat"]
        assert np.array_equal(_flat(a["model"]), _flat(b["model"])), f"{cs}: f32 fast and compat loops see the same images: bit-identical"
    monkeypatch.chdir(tmp_path)                   # opt.save is part of the checkpoint: a relative directory, the same for every run
    r = pretrain_g.main(RGB_ARGS + ["--save", "rgb_out"])
    digest = hashlib.sha256(open(r["path"], "rb").read()).hexdigest()
    assert digest == open(GOLDEN).read().split()[0], "pretrain_g --colorSpace rgb no longer writes the checkpoint it wrote before"
