"""gpu: nn.SpatialAveragePooling(2,2,2,2) (GR_AVGPOOL2) on the device against the split oracle (tests/avgpool_oracle.py), and
pretrain_g.lua's autoencoder loop (ganrev.pretrain_g) with the pretrained-G hand-over to ganrev.train."""
import os

import numpy as np
import pytest

import ganrev._lib as L
from ganrev import models, nn, pretrain_g, synth, t7, train
from avgpool_oracle import SplitOracle, adopt_device_choices, inject_masks
from helpers import TOL, assert_close, assert_grads_close

pytestmark = pytest.mark.gpu


def _stage(kind, cin, c, drop_after=False):
    m = nn.Sequential()
    if kind == "bn_relu":                  # create_G_encoder's first block (models.lua:68-71)
        m.add(nn.SpatialConvolution(cin, c, 3, 3, 1, 1, 1, 1)); m.add(nn.SpatialBatchNormalization(c)); m.add(nn.ReLU())
        m.add(nn.SpatialAveragePooling(2, 2, 2, 2))
        if drop_after:
            m.add(nn.Dropout(0.5))
    else:                                  # create_D_default's blocks (models.lua:231-235): conv - PReLU | SpatialDropout - AvgPool
        m.add(nn.SpatialConvolution(cin, c, 3, 3, 1, 1, 1, 1)); m.add(nn.PReLU()); m.add(nn.SpatialDropout(0.25))
        m.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    return m


def _consumer(m, c):
    """a 3x3 convolution behind the pool (its input the operand-ready image when the P16 path is on: conv_p16_supported wants 64
    output channels), and a BatchNorm so that the pool stage's own backward gets its dy operand-ready"""
    m.add(nn.SpatialConvolution(c, 64, 3, 3, 1, 1, 1, 1)); m.add(nn.SpatialBatchNormalization(64)); m.add(nn.ReLU())
    return m


def _run(oracle, model, dims, B, seed, training=True, max_flips=4):
    synth.init_params(model, seed)
    for m in model.leaves():
        if m.typename == "nn.PReLU":
            m.weight[...] = 0.25            # nn.PReLU's initial slope (a positive slope: the side of zero shows in the output)
    # an already compiled net keeps the BatchNorm running statistics its earlier training-mode forwards moved: the host values the
    # oracle is built from go to the device too (what evaluate() normalises with)
    model.push_params()
    so = SplitOracle(oracle, model, dims)
    x = synth.uniform((B,) + dims, seed + 1, -1, 1)
    (model.training() if training else model.evaluate()); so.set_training(training)
    if training:
        inject_masks(model, so, B, seed)
    out = model.forward(x)
    ref = so.forward(x)
    adopt_device_choices(model, so, B, max_flips)
    if training:
        inject_masks(model, so, B, seed)
    ref = so.forward(x)
    assert_close(out, ref, TOL * max(1.0, float(np.abs(ref).max())), f"forward ({'training' if training else 'evaluate'})")
    if not training:
        return out, ref, so
    gy = synth.normal(ref.shape, seed + 2) * np.float32(0.1)
    flat, grads = model.getParameters()
    grads[...] = 0; so.zero_grads()
    gin = model.backward(x, gy)
    ref_gin = so.backward(gy)
    assert_close(gin, ref_gin, TOL * max(1.0, float(np.abs(ref_gin).max())), "gradInput")
    assert_grads_close(model, grads, so.grads, what="avgpool")
    return out, ref, so


@pytest.mark.parametrize("kind,cin,c,H,W,drop", [
    ("bn_relu", 3, 16, 9, 7, False),       # odd extents: scalar kernels, floor as THNN
    ("bn_relu", 3, 16, 16, 16, True),      # float4 kernels, Dropout behind the pool
    ("bn_relu", 16, 32, 32, 32, False),
    ("prelu", 3, 16, 16, 16, False),       # PReLU closes its stage; SpatialDropout - AvgPool is an element-wise stage
    ("prelu", 16, 8, 10, 6, False)])
def test_avgpool_stage_matches_split_oracle(oracle, conv_mode, kind, cin, c, H, W, drop):
    for training in (True, False):
        model = _stage(kind, cin, c, drop)
        _run(oracle, model, (cin, H, W), 3, 11, training)


def test_avgpool_operand_ready_kernels(oracle, ctx, f16_path):
    """>= 64 channels at 32x32 with a consumer convolution: with p16_min_tiles = 1 the pool stage runs post_forward_g8_kernel and
    the operand-ready pass B with the average pool; results as the split oracle; evaluate() with eval_p16 on and off agree."""
    dims, B = (1, 32, 32), 8          # as test_R_operand_ready_path_vs_oracle: a few-input first stage writes the pool stage's input operand-ready
    model = nn.Sequential()
    model.add(nn.SpatialConvolution(1, 64)); model.add(nn.SpatialBatchNormalization(64)); model.add(nn.ReLU())
    for m in _stage("bn_relu", 64, 64).modules:
        model.add(m)
    model = _consumer(model, 64)
    synth.init_params(model, 5)
    ctx.set_timing(2)
    try:
        _run(oracle, model, dims, B, 5, True)
        kt = ctx.kernel_times()
    finally:
        ctx.set_timing(0)
    count = lambda prefix: sum(k["launches"] for k in kt if k["kernel"].startswith(prefix))
    if f16_path.endswith("p16"):
        assert count("post_forward_g8_kernel") >= 1 and count("post_backward_b_g8_kernel") >= 1, sorted((k["kernel"], k["launches"]) for k in kt)
    x = synth.uniform((B,) + dims, 6, -1, 1)
    model.evaluate()
    outs = []
    for v in (1, 0):
        ctx.set_tuning("eval_p16", v)
        outs.append(model.forward(x).copy())
    ctx.set_tuning("eval_p16", 1)
    assert_close(outs[0], outs[1], 2e-5, "evaluate(): eval_p16 on vs off")
    _run(oracle, model, dims, B, 5, False)


def test_avgpool_has_no_pool_index(ctx):
    model = _stage("bn_relu", 3, 8)
    synth.init_params(model, 1)
    model.training()
    model.forward(synth.uniform((2, 3, 8, 8), 1, 0, 1))
    buf = np.empty(2 * 8 * 4 * 4, np.uint8)
    rc = model._net.lib.gr_net_get_pool_index(model._net.h, 3, L._ptr(buf), buf.size)
    assert rc == -1                         # GR_ERR_INVALID: an average pool keeps no argmax
    assert model._net.layer_output(3, (buf.size,)).shape == (buf.size,)     # gr_net_layer_output works on the new layer


@pytest.mark.parametrize("dims,B,near_tie", [((1, 32, 32), 4, 1e-4), ((3, 64, 64), 8, 5e-4)])
def test_autoencoder_step_matches_split_oracle(oracle, conv_mode, dims, B, near_tie):
    """pretrain_g.lua's G_AUTOENCODER: forward, MSE against the input, backward and one penalty-clamp-Adam step.  At 64x64 the
    decoder's 1-D BatchNorm normalises differences of a few samples, ten layers deep: its ReLU inputs carry up to ~3e-4 of rounding
    (measured in all three arithmetics at two images), so a kink within 5e-4 of zero may legitimately fall on either side"""
    nd = 16
    ae = pretrain_g.build(dims, nd, 3)
    synth.init_params(ae, 3)
    so = SplitOracle(oracle, ae, dims)
    x = synth.uniform((B,) + dims, 4, 0, 1)
    ae.training(); so.set_training(True)
    out = ae.forward(x)
    so.forward(x)
    adopt_device_choices(ae, so, B, 8, near_tie, rel_flips=1e-4)
    ref = so.forward(x)
    assert_close(out, ref, TOL, "autoencoder forward")
    loss, g = ae._context().mse(out, x)
    rloss, rg = oracle.mse(ref, x)
    assert abs(loss - rloss) <= 1e-5 * max(1.0, abs(rloss))
    ae._net.zero_grads(); so.zero_grads()
    ae._net.backward(x, g, want_gin=False)
    so.backward(rg)
    got = ae._net.get_grads()
    assert_grads_close(ae, got, so.grads, what="autoencoder")
    theta = so.params.copy()
    hyper = L.Hyper(l1=0.0, l2=0.0, clamp=5.0)
    ae._net.adam_reset()
    ae._net.adam_step(hyper, 1)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    oracle.penalty_clamp_adam(theta, so.grads.copy(), m, v, oracle.GoHyper(l1=0.0, l2=0.0, clamp=5.0), 1)
    # Adam's first step moves every parameter by ~lr * sign(g): a gradient that is rounding residue on both sides (a bias in front
    # of BatchNorm) may take either sign, so the step is compared where the oracle's gradient is not residue
    sig = np.abs(so.grads) > 1e-4 * max(1e-3, float(np.abs(so.grads).max()))
    assert_close(ae._net.get_params()[sig], theta[sig], 2e-5, "parameters after one Adam step")


@pytest.mark.parametrize("builder", [models.create_D_default, models.create_D_facegen])
def test_average_pool_discriminators_match_split_oracle(oracle, conv_mode, builder):
    model = builder((3, 32, 32), True, 7)
    _run(oracle, model, (3, 32, 32), 2, 7, True)


def _small_opts(tmp_path, extra=()):
    return ["--epochs", "1", "--N_epoch", "1", "--batchSize", "4", "--noiseDim", "16", "--colorSpace", "y", "--save", str(tmp_path),
            "--saveFreq", "1", "--quiet"] + list(extra)


def test_pretrain_fast_matches_compat(ctx, conv_mode, tmp_path):
    """one batch, fast loop against the fevalG closure over optim.adam, from identical state; the bar of
    test_device_resident_gan_batch_matches_the_host_mirror.  Adam's first step is ~lr * sign(g): where the true gradient is exactly
    zero - a convolution / Linear bias in front of BatchNorm - both sides hold rounding residue of either sign and may step by
    +-lr in opposite directions (|dtheta| <= 2 lr); everywhere else the two agree to the last bits."""
    from helpers import param_segments
    res = [pretrain_g.main(_small_opts(tmp_path / k, ["--conv-mode", conv_mode] + (["--compat"] if k == "compat" else []))) for k in ("fast", "compat")]
    fast, compat = res[0]["model"], res[1]["model"]
    pf = (fast._flat_host() if fast._flat is None else fast._flat[0]).astype(np.float64)
    pc = compat._flat[0].astype(np.float64)
    d = np.abs(pf - pc)
    print(f"[pretrain fast vs compat] {conv_mode}: max |dtheta| {d.max():.3e} ({'bit-identical' if d.max() == 0 else 'not bit-identical'})")
    assert abs(res[0]["last_loss"] - res[1]["last_loss"]) <= 1e-5 * max(1.0, abs(res[1]["last_loss"]))
    leaves = compat.leaves()
    residue = np.zeros(d.size, bool)
    for mod, nm, lo, hi in param_segments(compat):
        i = leaves.index(mod)
        if nm == "bias" and i + 1 < len(leaves) and leaves[i + 1].typename.endswith("BatchNormalization") and not mod.typename.endswith("BatchNormalization"):
            residue[lo:hi] = True
    if conv_mode != "f16x3":
        assert d.max() == 0, "f32 / bf16x6: the host entry points run the same kernels as the device loop: bit-identical"
        return
    # f16x3: the host entry points are range-guarded and keep fp32 copies of every tensor, so they select other kernels than the
    # device loop (no operand-ready hand-over): last-bit differences, which Adam's normalised first step turns into +-lr where a
    # gradient is within rounding of zero
    assert d.max() <= 2.1e-3, d.max()
    r = d[~residue]
    assert np.median(r) <= 1e-7 and (r > 1e-5).mean() <= 1e-2, (np.median(r), (r > 1e-5).mean())


def test_pretrain_script_hands_G_to_train(ctx, tmp_path):
    r = pretrain_g.main(["--epochs", "2", "--N_epoch", "2", "--batchSize", "4", "--noiseDim", "16", "--colorSpace", "rgb",
                         "--save", str(tmp_path), "--saveFreq", "1", "--quiet"])
    path = os.path.join(str(tmp_path), "g_pretrained_3x32x32_nd16.net")
    assert r["path"] == path and os.path.isfile(path)
    ck = t7.load_checkpoint(path)
    assert "_unconverted" not in ck and int(ck["EPOCH"]) == 3
    dec = r["model"].get(2)
    G = ck["G"]
    assert [m.typename for m in G.leaves()] == [m.typename.replace("cudnn.", "nn.") for m in dec.leaves()]
    for a, b in zip(G.leaves(), dec.leaves()):
        for pa, pb in zip(a.param_arrays(), b.param_arrays()):
            assert np.array_equal(pa, pb)
        if hasattr(b, "running_mean"):
            assert np.array_equal(a.running_mean, b.running_mean) and np.array_equal(a.running_var, b.running_var)
    common = ["--epochs", "1", "--N_epoch", "1", "--batchSize", "4", "--noiseDim", "16", "--colorSpace", "rgb", "--quiet",
              "--G_pretrained_dir", str(tmp_path)]
    theta = G._flat_host()
    seen = {}
    real = train.adversarial.make_env

    def spy(MODEL_G, *a, **k):
        seen["G"] = MODEL_G._flat_host().copy()
        return real(MODEL_G, *a, **k)
    train.adversarial.make_env = spy
    try:
        train.main(common + ["--save", str(tmp_path / "a")])
        assert np.array_equal(seen["G"], theta), "the game must start from the pretrained decoder"
        train.main(common + ["--save", str(tmp_path / "b"), "--nopretraining"])
        assert seen["G"].size == theta.size and not np.array_equal(seen["G"], theta)
    finally:
        train.adversarial.make_env = real
