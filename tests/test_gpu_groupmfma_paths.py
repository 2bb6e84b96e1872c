"""-m gpu: GR_GROUPCONV3 on the f16 / bf16 MFMA (csrc/groupmfma.hip) - every case of tests/groupmfma_paths.py as a one-stage net against
float64 with a per-element bound in both split arithmetics, the recorded labels against the mirror, += accumulation, bit-identity of a
second run and of an image run alone; the dispatch rule (f32 mode and the default tuning key keep today's kernels and today's bits); a
miniature create_G4 with 16-plane branches against the CPU oracle; the full create_G4 at the default key, bundle against parts route.

Every test that moves `group_mfma_min_tiles` or the arithmetic restores the mirror's default and the previous mode in `finally`."""
import numpy as np
import pytest

import ganrev._lib as L
import groupmfma_paths as gm
from ganrev import models, synth
from g4_oracle import G4Oracle, KINK_GAP, mini_g4, pick_seed
from helpers import TOL, assert_close, assert_grads_close

pytestmark = pytest.mark.gpu
KEY = "group_mfma_min_tiles"
NEVER = 1 << 30


def _pass(net, x, gout):
    out = net.forward(x).copy()
    net.zero_grads()
    gin = net.backward(x, gout).copy()
    return out, gin, net.get_grads()


def _timed_pass(ctx, net, x, gout):
    ctx.set_timing(2)
    try:
        res = _pass(net, x, gout)
        names = {t["kernel"] for t in ctx.kernel_times()}
    finally:
        ctx.set_timing(0)
    return res, names & gm.UNIVERSE


def _net(ctx, case):
    d = gm.inputs(case.name)
    net = L.Net(ctx, case.descs(), case.dims)
    assert net.n_params == d["params"].size and tuple(net.out_dims) == (case.C, case.H, case.W)
    net.set_params(d["params"])
    return net, d


@pytest.mark.parametrize("mode", gm.MODES)
@pytest.mark.parametrize("case", gm.CASES, ids=[c.name for c in gm.CASES])
def test_groupmfma_path_within_float64_bound(ctx, case, mode):
    ref = gm.reference(case.name, mode)
    prev = ctx.conv_mode()
    net, d = _net(ctx, case)
    x, gout = d["x"], d["gout"]
    try:
        ctx.set_conv_mode(mode)
        ctx.set_tuning(KEY, 1)
        got = _pass(net, x, gout)
        timed, ran = _timed_pass(ctx, net, x, gout)
        net.backward(x, gout)
        twice = net.get_grads()
    finally:
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        ctx.set_conv_mode(prev)
        net.close()
    out, gin, grads = got
    tensors = {"out": out, "gin": gin, "gw": grads[:case.n_weights].reshape(ref["gw"][0].shape)}
    worst = {k: float(gm.ratio(v, ref[k][0], ref[k][1]).max()) for k, v in tensors.items()}        # print every figure, then assert
    print(f"{case.name} {mode}: max |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in tensors.items():
        gm.check_bound(v, ref[k][0], ref[k][1], f"{case.name} {mode} {k}")
    assert ran == case.labels(mode, 1) == set(gm.MFMA_LABELS), f"{case.name}: the net launched {sorted(ran)}; the mirror predicts {sorted(case.labels(mode, 1))}"
    for what, a, b in zip(("output", "gradInput", "gradients"), got, timed):
        assert np.array_equal(a, b), f"{case.name} {mode} {what}: a second run differs from the first"
    assert np.array_equal(twice, grads + grads), f"{case.name} {mode}: a second backward is not g1 + g1 (max diff {float(np.abs(twice - 2 * grads).max()):.3e})"
    if 0.0 in case.amps:                                       # a tile of zeros: exactly the bias, exactly no gradient
        z = case.amps.index(0.0)
        assert np.array_equal(out[z], np.broadcast_to(d["b"][:, None, None], out[z].shape)) and not np.any(gin[z])


def test_an_image_does_not_depend_on_the_batch_around_it(ctx):
    """f16x3 scales per (image, group) tile: forward and gradInput of gm_mini's three images equal, bit for bit, each image run alone"""
    case = gm.BY_NAME["gm_mini"]
    prev = ctx.conv_mode()
    net, d = _net(ctx, case)
    try:
        ctx.set_conv_mode("f16x3")
        ctx.set_tuning(KEY, 1)
        out, gin, _ = _pass(net, d["x"], d["gout"])
        for i in range(case.B):
            (o1, g1, _), ran = _timed_pass(ctx, net, d["x"][i:i + 1], d["gout"][i:i + 1])
            assert ran == set(gm.MFMA_LABELS)
            assert np.array_equal(o1[0], out[i]) and np.array_equal(g1[0], gin[i]), f"image {i} alone differs from image {i} in the batch"
    finally:
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        ctx.set_conv_mode(prev)
        net.close()


def test_f32_mode_keeps_the_fp32_kernels_and_their_bits(ctx):
    case = gm.BY_NAME["gm_mini"]
    prev = ctx.conv_mode()
    net, d = _net(ctx, case)
    try:
        ctx.set_conv_mode("f32")
        ctx.set_tuning(KEY, 1)
        forced, ran = _timed_pass(ctx, net, d["x"], d["gout"])
        assert ran == case.labels("f32", 1) == set(gm.FP32_LABELS), sorted(ran)
        ctx.set_tuning(KEY, NEVER)
        today = _pass(net, d["x"], d["gout"])
        ctx.set_conv_mode("f16x3")
        today_f16 = _pass(net, d["x"], d["gout"])
    finally:
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        ctx.set_conv_mode(prev)
        net.close()
    for what, a, b, c in zip(("output", "gradInput", "gradients"), forced, today, today_f16):
        assert np.array_equal(a, b) and np.array_equal(a, c), f"{what}: f32 mode with the key at 1 differs from the fp32 kernels' result"


@pytest.mark.parametrize("mode", gm.MODES)
def test_default_key_keeps_small_batches_on_the_fp32_kernels(ctx, mode):
    case = gm.BY_NAME["gm_mini"]
    prev = ctx.conv_mode()
    net, d = _net(ctx, case)
    try:
        ctx.set_conv_mode(mode)
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        default, ran = _timed_pass(ctx, net, d["x"], d["gout"])
        assert ran == case.labels(mode, gm.DEFAULT_MIN_TILES) == set(gm.FP32_LABELS), sorted(ran)
        ctx.set_tuning(KEY, NEVER)
        never = _pass(net, d["x"], d["gout"])
    finally:
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        ctx.set_conv_mode(prev)
        net.close()
    for what, a, b in zip(("output", "gradInput", "gradients"), default, never):
        assert np.array_equal(a, b), f"{what}: the default key differs from the key at 2^30"


# ---------------------------------------------------------------------------------------------------------------- integration
ND, B = 5, 3
_SEED = {}


def _mini(bundle=True):
    """create_G4 in small with 16-plane branches: nb = 2; Linear(5, 4) - PReLU - Linear(4, 256) - BatchNorm - PReLU - Reshape(16, 4, 4) - up-sampling -
    conv 16 -> 16 - BatchNorm - PReLU; tail conv 32 -> 4 - BatchNorm - PReLU - conv 4 -> 1 - Sigmoid"""
    return mini_g4(nb=2, nd=ND, hidden=4, planes=16, side=4, tail=4, bundle=bundle)


@pytest.mark.parametrize("mode", gm.MODES)
def test_miniature_bundle_on_the_mfma_kernels_vs_oracle(oracle, ctx, mode):
    """test_gpu_g4.test_miniature_vs_oracle's checks and bars with the grouped convolution on the MFMA launches (key = 1): training forward,
    gradInput, every parameter gradient, the running statistics, the evaluate() forward"""
    if "mini" not in _SEED:                                  # (on a twin of its own: every forward it tries moves the running statistics)
        _SEED["mini"] = pick_seed(G4Oracle(oracle, _mini(False), (ND, 1, 1)), (B, ND), True)[0]
    seed = _SEED["mini"]
    og = G4Oracle(oracle, _mini(False), (ND, 1, 1))
    x = synth.normal((B, ND), seed)
    prev = ctx.conv_mode()
    try:
        ctx.set_conv_mode(mode)
        ctx.set_tuning(KEY, 1)
        model = _mini()
        assert model.children() is None and len(model._param_chunks()) == 1
        flat, grads = model.getParameters()
        assert np.array_equal(og.params, flat)
        model.training(); og.set_training(True)
        ref = og.forward(x)
        gap = og.min_kink_distance()
        gy = synth.normal(ref.shape, 9)
        ctx.set_timing(2)
        try:
            out = model.forward(x).copy()
            grads[...] = 0; og.zero_grads()
            gin = model.backward(x, gy)
            ran = {t["kernel"] for t in ctx.kernel_times()} & gm.UNIVERSE
        finally:
            ctx.set_timing(0)
        print(f"[mini G4 16 planes {mode}] input seed {seed}: smallest |PReLU input| {gap:.2e}, out {float(np.abs(out - ref).max()):.2e}; ran {sorted(ran)}")
        assert ran == set(gm.MFMA_LABELS), sorted(ran)
        assert gap >= KINK_GAP and out.shape == (B, 1, 8, 8)
        assert_close(out, ref, TOL, "training forward")
        ref_gin = og.backward(x, gy)
        assert_close(gin, ref_gin, TOL * float(np.abs(ref_gin).max()), "gradInput")
        assert_grads_close(model, grads, og.grads, 1e-4, 1e-3, f"mini G4 16 planes {mode}")
        model.pull_params()
        stats = og.bn_running()
        bns = [m for m in model.leaves() if hasattr(m, "running_mean")]
        assert len(stats) == len(bns) == 5
        for m, (_, rm, rv) in zip(bns, stats):
            assert_close(m.running_mean, rm, TOL, f"{m.typename} running_mean"); assert_close(m.running_var, rv, TOL, f"{m.typename} running_var")
        model.evaluate(); og.set_training(False)
        ctx.set_timing(2)
        try:
            out = model.forward(x).copy()
            ran = {t["kernel"] for t in ctx.kernel_times()} & gm.UNIVERSE
        finally:
            ctx.set_timing(0)
        assert ran == {"groupconv3_mfma_forward_kernel"}, sorted(ran)
        assert_close(out, og.forward(x), TOL, "evaluate() forward")
    finally:
        ctx.set_timing(0)
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        ctx.set_conv_mode(prev)


def test_full_model_takes_the_mfma_forward_at_the_default_key(ctx):
    """create_G4((1, 32, 32), 32) at B = 16 (512 tiles), f16x3, evaluate(): the bundle records the MFMA forward and lies within TOL of the
    parts route on the same parameters (which test_gpu_g4.py holds to the oracle)"""
    x = synth.normal((16, 32), 8)
    prev = ctx.conv_mode()
    res = {}
    try:
        ctx.set_conv_mode("f16x3")
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        for route in ("bundle", "parts"):
            G = synth.init_params(models.create_G4((1, 32, 32), 32, seed=6), 7)
            if route == "parts":
                G.modules[1].bundle = False
            G.evaluate()
            ctx.set_timing(2)
            try:
                res[route] = G.forward(x).copy()
                ran = {t["kernel"] for t in ctx.kernel_times()} & gm.UNIVERSE
            finally:
                ctx.set_timing(0)
            assert ran == ({"groupconv3_mfma_forward_kernel"} if route == "bundle" else set()), (route, sorted(ran))
    finally:
        ctx.set_timing(0)
        ctx.set_tuning(KEY, gm.DEFAULT_MIN_TILES)
        ctx.set_conv_mode(prev)
    print(f"[create_G4 B = 16 f16x3] bundle vs parts {float(np.abs(res['bundle'] - res['parts']).max()):.2e}")
    assert_close(res["bundle"], res["parts"], TOL, "evaluate() forward, bundle vs parts")
