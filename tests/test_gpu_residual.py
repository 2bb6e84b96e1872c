"""GPU: the pointwise convolution (csrc/conv1x1.hip) and models.createResidual (reference models.lua:8-55) against the CPU oracle, in
all three convolution arithmetics - the 1x1 kernels are exact fp32 in each, their 3x3 neighbours are not.

The project's bars: outputs within 1e-4 absolute, every gradient tensor within 1e-4 of its module's largest entry
(helpers.assert_grads_close), gradInput within 1e-4 of its largest entry.  The block cases choose their input on the CPU
(residual_oracle.pick_seed): the first seed whose oracle forward keeps every ReLU / LeakyReLU / PReLU input 1e-5 away from zero.

The library (as the oracle) refuses a backward through BatchNormalization in evaluate() mode, so the evaluate() halves of the cases
with BatchNorm compare the forward, and the case without BatchNorm the backward as well."""
import numpy as np
import pytest

import ganrev._lib as L
from ganrev import device, models, nn, synth
from helpers import TOL, assert_close, assert_grads_close
from residual_oracle import ResidualOracle, conv1x1_reference, pick_seed

pytestmark = pytest.mark.gpu

C1_KERNELS = {"conv1x1_kernel", "conv1x1_kernel(dgrad)", "conv1x1_wgrad_kernel", "conv1x1_wgrad_reduce_kernel"}

# (B, Cin, Cout, H, W): nothing aligned | whole tiles | HW below a pixel tile | more images than batch splits | odd HW, Cout past one tile
OPERATOR_CASES = [(3, 5, 7, 6, 10), (2, 64, 32, 8, 8), (4, 32, 64, 4, 4), (70, 16, 16, 4, 4), (1, 3, 130, 5, 5)]


@pytest.mark.parametrize("B,Cin,Cout,H,W", OPERATOR_CASES)
def test_conv1x1_alone_vs_oracle(oracle, ctx, conv_mode, B, Cin, Cout, H, W):
    """A one-layer net GR_CONVK c = 1: forward, gradInput, gradWeight and gradBias against go_convk_* with K = 1; a second backward
    without zero_grads doubles the gradients exactly (+=); a second run gives the same bits; the conv1x1_* kernels ran and no
    convk_direct* kernel did."""
    net = L.Net(ctx, [(L.CONVK, Cin, Cout, 1, 0.0, 0)], (Cin, H, W))
    try:
        s = 1.0 / np.sqrt(Cin)
        w, b = synth.uniform((Cout, Cin), 3, -s, s), synth.uniform((Cout,), 4, -0.5, 0.5)
        x, gout = synth.normal((B, Cin, H, W), 5), synth.normal((B, Cout, H, W), 6)
        assert net.n_params == w.size + b.size
        net.set_params(np.concatenate([w.ravel(), b]))
        ref_out, ref_gin, ref_gw, ref_gb = conv1x1_reference(oracle, x, w, b, gout)
        ctx.set_timing(2)
        out = net.forward(x).copy()
        net.zero_grads()
        gin = net.backward(x, gout).copy()
        names = {k["kernel"] for k in ctx.kernel_times()}
        ctx.set_timing(0)
        g1 = net.get_grads()
        assert C1_KERNELS <= names and not any(n.startswith("convk_direct") for n in names), sorted(names)
        d_out = float(np.abs(out - ref_out).max())
        d_gin = float(np.abs(gin - ref_gin).max()) / float(np.abs(ref_gin).max())
        ref_g = np.concatenate([ref_gw.ravel(), ref_gb])
        gmax = float(np.abs(ref_g).max())
        d_gw = float(np.abs(g1[:w.size] - ref_gw.ravel()).max()) / gmax
        d_gb = float(np.abs(g1[w.size:] - ref_gb).max()) / gmax
        print(f"[conv1x1 {B}x{Cin}->{Cout} {H}x{W} {conv_mode}] out {d_out:.2e}  gin {d_gin:.2e}  gw {d_gw:.2e}  gb {d_gb:.2e} (relative to max |g| {gmax:.3g})")
        assert d_out <= TOL and d_gin <= TOL and d_gw <= 1e-4 and d_gb <= 1e-4
        net.backward(x, gout)                       # accGradParameters: += into what the first backward left
        g2 = net.get_grads()
        assert np.array_equal(g2, g1 + g1), float(np.abs(g2 - 2 * g1).max())
        out_b = net.forward(x)
        net.zero_grads()
        gin_b = net.backward(x, gout)
        assert np.array_equal(out_b, out) and np.array_equal(gin_b, gin) and np.array_equal(net.get_grads(), g1)
    finally:
        ctx.set_timing(0)
        net.close()


def test_convk_other_windows_are_still_refused(ctx):
    with pytest.raises(L.GanrevError) as e:
        L.Net(ctx, [(L.CONVK, 4, 4, 7, 0.0, 0)], (4, 8, 8))
    # (the wording is the one tests/test_gpu_net_memory.py pins: it names the 3x3 and 5x5 windows)
    assert "GR_ERR_UNSUPPORTED" in str(e.value) and "7x7" in str(e.value) and "3x3" in str(e.value) and "5x5" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- inside a stage
def _stage_model():
    """1x1 -> SpatialBatchNormalization -> PReLU -> 3x3: the hand-over to a 3x3 kernel, BatchNorm statistics over a 1x1 output"""
    m = nn.Sequential()
    m.add(nn.SpatialConvolution(8, 16, 1, 1, 1, 1, 0, 0))
    m.add(nn.SpatialBatchNormalization(16))
    m.add(nn.PReLU())
    m.add(nn.SpatialConvolution(16, 16, 3, 3, 1, 1, 1, 1))
    return synth.init_params(m, 31)


def _nested_model():
    """a 3x3 stage, a block, View -> Linear: the block as one part between two compiled chunks"""
    m = nn.Sequential()
    m.add(nn.SpatialConvolution(3, 8, 3, 3, 1, 1, 1, 1))
    m.add(nn.SpatialBatchNormalization(8))
    m.add(nn.ReLU())
    m.add(models.createResidual(8, 4, 8, "PReLU"))
    m.add(nn.View(8 * 8 * 8))
    m.add(nn.Linear(8 * 8 * 8, 5))
    return synth.init_params(m, 32)


BLOCK_CASES = [(16, 16, 16, "ReLU", True), (16, 8, 16, "PReLU", True), (8, 8, 16, "LeakyReLU", True), (6, 12, 10, "ReLU", False)]
B, HW = 4, 8


def _block(i):
    a, inner, c, act, bn = BLOCK_CASES[i]
    return synth.init_params(models.createResidual(a, inner, c, act, bn), 40 + i), (a, HW, HW), bn


def _check_vs_oracle(oracle, model, dims, has_bn, what):
    og = ResidualOracle(oracle, model, dims)
    flat, grads = model.getParameters()
    assert np.array_equal(og.params, flat)
    for training in (True, False):
        (model.training if training else model.evaluate)()
        seed, x, ref = pick_seed(og, (B,) + dims, training)
        out = model.forward(x)
        d = float(np.abs(out - ref).max())
        print(f"[{what} {'training' if training else 'evaluate'}] input seed {seed}: kink distance {og.min_kink_distance():.2e}, out {d:.2e}")
        assert_close(out, ref, TOL, f"{what} forward ({'training' if training else 'evaluate'})")
        if not training and has_bn:
            continue
        gy = synth.normal(ref.shape, 9)
        grads[...] = 0; og.zero_grads()
        gin = model.backward(x, gy)
        ref_gin = og.backward(x, gy)
        assert gin.shape == x.shape
        assert_close(gin, ref_gin, TOL * float(np.abs(ref_gin).max()), f"{what} gradInput")
        assert_grads_close(model, grads, og.grads, 1e-4, 1e-3, what)


def test_conv1x1_inside_a_stage_vs_oracle(oracle, conv_mode):
    _check_vs_oracle(oracle, _stage_model(), (8, HW, HW), True, "1x1-BN-PReLU-3x3")


@pytest.mark.parametrize("case", range(len(BLOCK_CASES)), ids=["same", "bottleneck", "widen", "all-different-no-bn"])
def test_residual_block_vs_oracle(oracle, conv_mode, case):
    model, dims, bn = _block(case)
    kinds = [type(p).__name__ for p in model.parts()]
    assert kinds == ["_TableSum"], kinds
    _check_vs_oracle(oracle, model, dims, bn, f"createResidual{BLOCK_CASES[case]}")


# ---------------------------------------------------------------------------------------------------------------- device-resident
def _flat_dev(dm, what):
    return np.concatenate([getattr(n, what)() for n in dm.nets])


def _device_equals_host(oracle, ctx, model, dims, seed):
    """DeviceModel forward / backward = the host containers bit for bit (output, gradInput, flat gradient): the same nets run the same
    kernels, the sums are the same float32 additions in the same order.  Then one Adam step on the device model against the oracle's
    penalty_clamp_adam on the same gradients (the bit-exact rule gr_adam_step is held to)."""
    x, Bn = synth.normal((B,) + dims, seed), B
    model.training()
    flat, grads = model.getParameters()
    out = model.forward(x).copy()
    gy = synth.normal(out.shape, 9)
    grads[...] = 0
    gin = model.backward(x, gy).copy()
    g_host = grads.copy()
    dm = device.DeviceModel(ctx, model)
    xd, gd = ctx.upload(x), ctx.upload(gy)
    try:
        assert len(dm.nets) == len(model._param_chunks()) >= 1
        dm.set_training(True)
        for _ in range(2):          # twice: the executor's buffers are reused, nothing of the first step may leak into the second
            dm.zero_grads()
            od = dm.forward(xd, Bn)
            out_d = ctx.download(od, out.shape)
            gind = dm.backward(gd, Bn, True)
            gin_d = ctx.download(gind, x.shape)
            assert np.array_equal(out_d, out), float(np.abs(out_d - out).max())
            assert np.array_equal(gin_d, gin), float(np.abs(gin_d - gin).max())
            assert np.array_equal(_flat_dev(dm, "get_grads"), g_host)
        live = dict(dm.mem.nbytes)
        dm.forward(xd, Bn); dm.backward(gd, Bn, True)
        assert dm.mem.nbytes == live            # nothing allocated per step
        theta = _flat_dev(dm, "get_params")
        assert np.array_equal(theta, flat)
        dm.adam_reset()
        dm.zero_grads(); dm.forward(xd, Bn); dm.backward(gd, Bn, False)
        dm.adam_step(L.Hyper(l1=0.0, l2=0.0, clamp=0.0), 1)
        m, v = np.zeros_like(theta), np.zeros_like(theta)
        oracle.penalty_clamp_adam(theta, g_host.copy(), m, v, oracle.GoHyper(l1=0.0, l2=0.0, clamp=0.0), 1)
        assert np.array_equal(_flat_dev(dm, "get_params"), theta)
        dm.set_training(False)
        assert not any(n.training for n in dm.nets)
        dm.range_guard_scan()
    finally:
        ctx.free(xd); ctx.free(gd); dm.close()


@pytest.mark.parametrize("case", range(len(BLOCK_CASES)), ids=["same", "bottleneck", "widen", "all-different-no-bn"])
def test_device_model_equals_host_containers_block(oracle, ctx, conv_mode, case):
    model, dims, _ = _block(case)
    _device_equals_host(oracle, ctx, model, dims, 3)


def test_device_model_equals_host_containers_nested(oracle, ctx, conv_mode):
    model = _nested_model()
    assert [type(p).__name__ for p in model.parts()] == ["Sequential", "Sequential", "Sequential"]
    assert [type(p).__name__ for p in model.parts()[1].parts()] == ["_TableSum"]
    _device_equals_host(oracle, ctx, model, (3, HW, HW), 4)


def test_device_model_of_a_single_stage_net(oracle, ctx, conv_mode):
    """case 2 (1x1 - BN - PReLU - 3x3) compiles to ONE net: the executor's trivial case, same bits as the host calls"""
    model = _stage_model()
    x = synth.normal((B, 8, HW, HW), 3)
    model.training()
    flat, grads = model.getParameters()
    out = model.forward(x).copy()
    gy = synth.normal(out.shape, 9)
    grads[...] = 0
    gin = model.backward(x, gy).copy()
    dm = device.DeviceModel(ctx, model)
    xd, gd = ctx.upload(x), ctx.upload(gy)
    try:
        dm.zero_grads()
        out_d = ctx.download(dm.forward(xd, B), out.shape)
        gin_d = ctx.download(dm.backward(gd, B, True), x.shape)
        assert np.array_equal(out_d, out) and np.array_equal(gin_d, gin) and np.array_equal(_flat_dev(dm, "get_grads"), grads)
    finally:
        ctx.free(xd); ctx.free(gd); dm.close()
