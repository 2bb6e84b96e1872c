"""-m gpu: the evaluate()-mode input gradient (gr_net_backward_input_dev), the row-wise criterion / optimiser and the refinement loop built
on them (ganrev.refine), against the float64 PyTorch reference of tests/refine_paths.py.

A  the frozen pipeline kernel alone (element-wise nets): every dy element within c * 2^-24 * |dy_ref|, c derived in refine_paths.c_bound
B  one- and two-stage nets in f32 / bf16x6 / f16x3: gradInput within 1e-4 * max|ref|; grads, running statistics, masks and the forward counter
   bit-unchanged by the call; the timer labels are the mirror's and hold no weight-gradient work
C  without BatchNorm the call repeats gr_net_backward_dev's gradInput bit for bit
D  d loss / d z of the whole G3 and G4
E  gr_mse_rows_dev / gr_adam_rows_step_dev
F  refine.refineNoise
G  the refusals and apply_r --refine

Cost: nets of at most a few thousand elements but for G4 (two images); the float64 references take under a second each, G4's a few."""
import json
import os

import numpy as np
import pytest

import refine_paths as rp
from helpers import TOL

pytestmark = pytest.mark.gpu


def _counts(ctx):
    out = {}
    for t in ctx.kernel_times():
        out[t["kernel"]] = out.get(t["kernel"], 0) + t["launches"]
    return out


def _make_net(ctx, case, d):
    import ganrev._lib as L
    net = L.Net(ctx, case.descs, case.dims)
    if net.n_params:
        net.set_params(d["params"])
    for i, (m, v) in enumerate(d["running"]):
        net.set_bn_running(i, m, v)
    net.set_training(False)
    return net


class _Dev:
    """device copies of a case's x and gradOutput and a gradInput buffer, freed on exit"""

    def __init__(self, ctx, x, gout):
        self.ctx, self.x, self.g, self.gin, self.shape = ctx, ctx.upload(x), ctx.upload(gout), ctx.malloc(x.nbytes), x.shape

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in (self.x, self.g, self.gin):
            self.ctx.free(p)

    def result(self):
        return self.ctx.download(self.gin, self.shape)


def _input_grad(net, d, dev, B, timed_ctx=None):
    """forward with the flag on (the case's always-on noise injected), then the input-only backward -> (gradInput, labels of the backward call)"""
    for li, keep in d["masks"].items():
        net.set_mask(li, keep)
    net.set_input_grad(True)
    net.forward_dev(dev.x, B)
    c0 = _counts(timed_ctx) if timed_ctx else None
    net.backward_input_dev(dev.x, dev.g, B, dev.gin)
    got = dev.result()
    ran = None
    if timed_ctx:
        c1 = _counts(timed_ctx)
        ran = {k for k in c1 if c1[k] - c0.get(k, 0) > 0}
    return got, ran


# ---------------------------------------------------------------------------------------------------------------- A
A_CASES = [c for c in rp.CASES if c.group == "A"]


@pytest.mark.parametrize("case", A_CASES, ids=[c.name for c in A_CASES])
def test_frozen_pipeline_alone_within_its_rounding_bound(ctx, case):
    d = rp.case_data(case.name)
    ref, c = d["ref"]["gin"], rp.c_bound(case)
    assert d["ref"]["zmax"] <= rp.Z_MAX
    ctx.set_conv_mode("f32")
    net = _make_net(ctx, case, d)
    try:
        with _Dev(ctx, d["x"], d["gout"]) as dev:
            got, _ = _input_grad(net, d, dev, case.B)
            ctx.set_timing(2)
            try:
                again, ran = _input_grad(net, d, dev, case.B, ctx)
            finally:
                ctx.set_timing(0)
    finally:
        net.close()
    rp.check_labels(ran, case.stages, "f32", case.B, case.name)
    assert np.array_equal(got, again), f"{case.name}: the timed pass differs"
    err, bound = np.abs(got.astype(np.float64) - ref), c * rp.U * np.abs(ref)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    print(f"{case.name}: c = {c:.1f}, worst |err| / (c u |ref|) = {ratio:.3f}, {int((ref == 0).sum())} of {ref.size} exact zeros")
    assert (err <= bound).all(), f"{case.name}: {int((err > bound).sum())} of {err.size} elements outside c u |dy_ref| (c = {c:.1f}); worst x{ratio:.2f}"


# ---------------------------------------------------------------------------------------------------------------- B
B_RUNS = [(c, m) for c in rp.CASES if c.group == "B" for m in rp.ALL_MODES]


@pytest.mark.parametrize("case,mode", B_RUNS, ids=[f"{c.name}-{m}" for c, m in B_RUNS])
def test_gradinput_of_small_nets_and_nothing_else_moves(ctx, case, mode):
    import ganrev._lib as L
    d = rp.case_data(case.name)
    ref = d["ref"]["gin"]
    ctx.set_conv_mode(mode)
    for k, v in case.tuning.items():
        ctx.set_tuning(k, v)
    net = _make_net(ctx, case, d)
    try:
        with _Dev(ctx, d["x"], d["gout"]) as dev:
            sentinel = np.random.default_rng(5).standard_normal(net.n_params).astype(np.float32)
            if net.n_params:
                net.set_grads(sentinel)
            net.set_input_grad(True)
            net.forward_dev(dev.x, case.B)
            before = ([net.get_bn_running(i) for i in range(net.n_bn())], net.forward_counter())
            ctx.set_timing(2)
            try:
                c0 = _counts(ctx)
                net.backward_input_dev(dev.x, dev.g, case.B, dev.gin)
                got = dev.result()
                c1 = _counts(ctx)
            finally:
                ctx.set_timing(0)
            ran = {k for k in c1 if c1[k] - c0.get(k, 0) > 0}
            after = ([net.get_bn_running(i) for i in range(net.n_bn())], net.forward_counter())
            if net.n_params:
                assert np.array_equal(net.get_grads(), sentinel), f"{case.name}: the flat gradient moved"
            assert before[1] == after[1]
            for (m0, v0), (m1, v1) in zip(before[0], after[0]):
                assert np.array_equal(m0, m1) and np.array_equal(v0, v1), f"{case.name}: a running statistic moved"
            net.backward_input_dev(dev.x, dev.g, case.B, dev.gin)                    # untimed, again: the same bits
            assert np.array_equal(dev.result(), got)
            if any(k[0] == L.BN for k in case.descs):
                with pytest.raises(L.GanrevError, match="requires training mode"):          # the full backward still refuses a frozen BatchNorm
                    net.backward_dev(dev.x, dev.g, case.B, dev.gin)
    finally:
        net.close()
        for k in case.tuning:
            ctx.set_tuning(k, rp.GROUP_MFMA_MIN_TILES)
    rp.check_labels(ran, case.stages, mode, case.B, case.name, case.tuning.get("group_mfma_min_tiles", rp.GROUP_MFMA_MIN_TILES))
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{case.name} [{mode}]: max |err| = {err:.3e} = {err / np.abs(ref).max():.2e} of max |ref|; ran {sorted(ran)}")
    assert err <= rp.GRAD_RTOL * np.abs(ref).max()


def test_masks_are_read_not_written(ctx):
    import ganrev._lib as L
    case = rp.BY_NAME["A-always-on-drop-8x8"]
    d = rp.case_data(case.name)
    ctx.set_conv_mode("f32")
    net = _make_net(ctx, case, d)
    try:
        with _Dev(ctx, d["x"], d["gout"]) as dev:
            _input_grad(net, d, dev, case.B)
            (li, keep), = d["masks"].items()
            assert np.array_equal(net.get_mask(li, keep.size), keep)
    finally:
        net.close()


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("mode", rp.ALL_MODES)
def test_without_batchnorm_the_bits_of_the_training_mode_backward(ctx, mode):
    case = rp.BY_NAME["C-no-bn"]
    d = rp.case_data(case.name)
    for st in case.stages:          # the mirror names the same data-gradient kernels on both routes: backward_impl's dgrad3 rule is dgrad_family's
        assert rp.dgrad_family(st, mode, case.B) in (None, "conv3_split" if mode != "f32" else "conv3_f32")
    ctx.set_conv_mode(mode)
    net = _make_net(ctx, case, d)
    try:
        with _Dev(ctx, d["x"], d["gout"]) as dev:
            net.set_training(True)
            net.forward_dev(dev.x, case.B)
            net.zero_grads()
            net.backward_dev(dev.x, dev.g, case.B, dev.gin)
            full = dev.result()
            net.set_training(False)
            got, _ = _input_grad(net, d, dev, case.B)
    finally:
        net.close()
    assert np.array_equal(got, full), f"[{mode}] {int((got != full).sum())} of {got.size} elements differ, max {np.abs(got - full).max():.3e}"
    assert np.abs(got.astype(np.float64) - d["ref"]["gin"]).max() <= rp.GRAD_RTOL * np.abs(d["ref"]["gin"]).max()


# ---------------------------------------------------------------------------------------------------------------- D
def _loss_gradient(ctx, G, z, images):
    """d (sum of the per-row MSE) / d z through the DeviceModel route the refinement takes"""
    from ganrev import device
    B, n = z.shape[0], images[0].size
    G.evaluate()
    G.forward(z)                                    # compiles
    dm = device.DeviceModel(ctx, G)
    zd, xd = ctx.upload(z), ctx.upload(images)
    gd, ld = ctx.malloc(4 * B * n), ctx.malloc(4 * B)
    try:
        dm.set_training(False)
        dm.set_input_grad(True)
        out = dm.forward(zd, B)
        ctx.mse_rows_dev(out, xd, B, n, ld, gd)
        gz = ctx.download(dm.backward(gd, B, True, params=False), z.shape)
        loss = ctx.download(ld, (B,))
    finally:
        dm.set_input_grad(False)
        for p in (zd, xd, gd, ld):
            ctx.free(p)
        dm.close()
    return loss, gz


def _loss_gradient64(fwd, z, images):
    import torch
    zz = torch.tensor(z.astype(np.float64), requires_grad=True)
    loss = ((fwd(zz).reshape(z.shape[0], -1) - torch.tensor(images.astype(np.float64)).reshape(z.shape[0], -1)) ** 2).mean(dim=1)
    loss.sum().backward()
    return loss.detach().numpy(), zz.grad.numpy()


@pytest.mark.parametrize("mode", rp.ALL_MODES)
def test_whole_g3_loss_gradient(ctx, mode):
    li = rp.loop_inputs()
    ctx.set_conv_mode(mode)
    G = rp.mini_g3(li["model_seed"])
    # (targets away from G's range: against li["images"] the residual G(z) - x is 1e-3 of the images and carries the forward's rounding at 1e-3 relative)
    z, images = np.ascontiguousarray(li["z0"][:5]), np.random.default_rng(2).uniform(0, 1, (5,) + rp.LOOP["dims"]).astype(np.float32)
    loss, gz = _loss_gradient(ctx, G, z, images)
    fwd = rp.build(li["descs"], (rp.LOOP["nd"], 1, 1), li["params"], li["running"])
    rloss, rgz = _loss_gradient64(fwd, z, images)
    err = float(np.abs(gz - rgz).max())
    print(f"G3 [{mode}]: max |err| {err:.3e} = {err / np.abs(rgz).max():.2e} of max |ref|; losses {loss} vs {rloss}")
    assert err <= rp.GRAD_RTOL * np.abs(rgz).max()
    assert np.abs(loss - rloss).max() <= 1e-4 * rloss.max()


@pytest.mark.parametrize("mode", rp.ALL_MODES)
def test_whole_g4_loss_gradient(ctx, mode):
    from ganrev import models, synth
    dims, nd, B = (3, 32, 32), 8, 2
    ctx.set_conv_mode(mode)
    G = models.create_G4(dims, nd, seed=3)
    synth.init_params(G, 3)
    rp.shake_running(G, 103)
    descs, flat, running = rp.model_spec(G, (nd, 1, 1))
    fwd = rp.build(descs, (nd, 1, 1), flat, running)
    rng = np.random.default_rng(3)
    z = rng.standard_normal((B, nd)).astype(np.float32)
    images = rng.uniform(0, 1, (B,) + dims).astype(np.float32)
    loss, gz = _loss_gradient(ctx, G, z, images)
    rloss, rgz = _loss_gradient64(fwd, z, images)
    err = float(np.abs(gz - rgz).max())
    print(f"G4 [{mode}]: max |err| {err:.3e} = {err / np.abs(rgz).max():.2e} of max |ref|")
    assert err <= rp.GRAD_RTOL * np.abs(rgz).max()
    assert np.abs(loss - rloss).max() <= 1e-4 * rloss.max()


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("rows,n", [(7, 77), (3, 4096)])
def test_mse_rows_against_float64_and_repeats(ctx, rows, n):
    rng = np.random.default_rng(rows)
    x, t = rng.standard_normal((rows, n)).astype(np.float32), rng.standard_normal((rows, n)).astype(np.float32)
    xd, td, ld, gd = ctx.upload(x), ctx.upload(t), ctx.malloc(4 * rows), ctx.malloc(4 * rows * n)
    try:
        ctx.mse_rows_dev(xd, td, rows, n, ld, gd)
        loss, grad = ctx.download(ld, (rows,)), ctx.download(gd, (rows, n))
        ctx.upload(np.zeros(rows, np.float32), ld)
        ctx.mse_rows_dev(xd, td, rows, n, ld, gd)
        assert np.array_equal(ctx.download(ld, (rows,)), loss) and np.array_equal(ctx.download(gd, (rows, n)), grad)
        ctx.upload(np.full((rows, n), 9.0, np.float32), gd)
        ctx.mse_rows_dev(xd, td, rows, n, ld, None)                              # grad_dev is nullable
        assert np.array_equal(ctx.download(ld, (rows,)), loss) and (ctx.download(gd, (rows, n)) == 9.0).all()
    finally:
        for p in (xd, td, ld, gd):
            ctx.free(p)
    z = (x - t).astype(np.float64)              # x - t is formed in fp32 by the kernel, as here; the squares and their sum in double
    rl = (z ** 2).mean(axis=1)
    assert np.abs(loss - rl).max() <= 2 * rp.U * rl.max()                        # the double sum rounded to fp32 once
    rg = 2.0 * z / n
    assert np.abs(grad - rg).max() <= 2 * rp.U * np.abs(rg).max()


def _adam_reference(theta, grads, lr):
    """optim.adam of ganrev/optim.py on the flat vector: three steps through the fused gr_adam_step of a Linear(4, 8) net (40 parameters)"""
    from ganrev import nn, optim, synth
    lin = nn.Linear(4, 8)
    lin.forward(synth.normal((1, 4), 3))
    assert lin._net.n_params == theta.size
    x, state, out = theta.copy(), {}, []
    for g in grads:
        optim.adam(lambda _: (0.0, g.copy()), x, {"learningRate": lr}, state, model=lin)
        out.append((x.copy(), state["m"].copy(), state["v"].copy()))
    lin._net.close()
    return out


def test_adam_rows_is_optim_adam_bit_for_bit_and_keeps_the_best(ctx):
    import ganrev._lib as L
    rows, nd, lr = 5, 8, 0.01
    rng = np.random.default_rng(11)
    z0 = rng.standard_normal((rows, nd)).astype(np.float32)
    grads = [(rng.standard_normal((rows, nd)) * 0.3).astype(np.float32) for _ in range(3)]
    ref = _adam_reference(z0.reshape(-1), [g.reshape(-1) for g in grads], lr)
    # per-row losses that rise and then fall (row 0), only rise (1), only fall (2), stay (3), NaN once (4)
    losses = np.array([[3, 5, 2, 1], [1, 2, 3, 4], [4, 3, 2, 1], [2, 2, 2, 2], [2, np.nan, 3, 1]], np.float32)
    zd, gd, md, vd = ctx.upload(z0), ctx.malloc(z0.nbytes), ctx.upload(np.zeros_like(z0)), ctx.upload(np.zeros_like(z0))
    ld, bd, bzd = ctx.malloc(4 * rows), ctx.upload(np.full(rows, np.inf, np.float32)), ctx.upload(np.full_like(z0, -7.0))
    hyper = L.AdamHyper(lr=lr)
    try:
        seen = [z0.copy()]
        for t in range(1, 4):
            ctx.upload(grads[t - 1], gd)
            ctx.upload(np.ascontiguousarray(losses[:, t - 1]), ld)
            ctx.adam_rows_step_dev(zd, gd, md, vd, rows, nd, hyper, t, ld, bd, bzd)
            z, m, v = (ctx.download(p, (rows, nd)) for p in (zd, md, vd))
            rz, rm, rv = (a.reshape(rows, nd) for a in ref[t - 1])
            assert np.array_equal(z, rz) and np.array_equal(m, rm) and np.array_equal(v, rv), f"step {t} differs from optim.adam"
            assert np.array_equal(ctx.download(gd, (rows, nd)), grads[t - 1])           # the gradient is read only
            seen.append(z.copy())
        ctx.upload(np.ascontiguousarray(losses[:, 3]), ld)
        ctx.adam_rows_step_dev(zd, None, None, None, rows, nd, None, 4, ld, bd, bzd, update=False)      # the last look
        for p, want in ((zd, seen[3]), (md, ref[2][1].reshape(rows, nd)), (vd, ref[2][2].reshape(rows, nd))):
            assert np.array_equal(ctx.download(p, (rows, nd)), want), "update = 0 moved z, m or v"
        best, best_z = ctx.download(bd, (rows,)), ctx.download(bzd, (rows, nd))
        # the z a loss belongs to is the one BEFORE that call's update: look t saw seen[t - 1]
        want_at = [3, 0, 3, 0, 3]
        assert np.array_equal(best, np.array([1, 1, 1, 2, 1], np.float32))
        for r, k in enumerate(want_at):
            assert np.array_equal(best_z[r], seen[k][r]), f"row {r}: best_z is not the z of look {k + 1}"
        # the clamp: a learning rate that throws every entry out of [-0.5, 0.5]
        ctx.upload(z0, zd); ctx.upload(np.zeros_like(z0), md); ctx.upload(np.zeros_like(z0), vd); ctx.upload(grads[0], gd)
        ctx.adam_rows_step_dev(zd, gd, md, vd, rows, nd, L.AdamHyper(lr=10.0), 1, ld, bd, bzd, clamp=0.5)
        z = ctx.download(zd, (rows, nd))
        assert (np.abs(z) == 0.5).all() and np.array_equal(np.sign(z), -np.sign(grads[0]))
    finally:
        for p in (zd, gd, md, vd, ld, bd, bzd):
            ctx.free(p)


# ---------------------------------------------------------------------------------------------------------------- F
def _refine(ctx, G, li, batch, mode="f16x3"):
    from ganrev import device, refine
    rows = rp.LOOP["rows"]
    G.evaluate()
    G.forward(li["z0"])
    dm = device.DeviceModel(ctx, G)
    zd, xd = ctx.upload(li["z0"]), ctx.upload(li["images"])
    try:
        state = lambda: [(n.forward_counter(), n.training, n.input_grad) for n in dm.nets]
        before = state()
        first, best = refine.refineNoise(ctx, dm, xd, zd, rows, rp.LOOP["steps"], batch, lr=rp.LOOP["lr"])
        assert state() == before, "refineNoise left a mode, a flag or a forward counter changed"
        return first, best, ctx.download(zd, li["z0"].shape)
    finally:
        ctx.free(zd); ctx.free(xd)
        dm.close()


@pytest.mark.parametrize("mode", rp.ALL_MODES)
def test_refine_noise_against_the_float64_loop(ctx, mode):
    li = rp.loop_inputs()
    r64 = li["r64"]
    ctx.set_conv_mode(mode)
    G = rp.mini_g3(li["model_seed"])
    probe = np.ascontiguousarray(li["z0"][:3])
    G.evaluate(); eval_before = G.forward(probe).copy()
    G.training(); train_before = G.forward(probe).copy(); G.push_bn_running()
    first, best, z = _refine(ctx, G, li, 6)
    assert (best <= first).all()                                                   # exact: a row never ends worse than it started
    assert (best < first).all(), "five steps towards the optimum improve every row of this input"
    again = _refine(ctx, G, li, 6)
    assert all(np.array_equal(a, b) for a, b in zip((first, best, z), again)), "a second run does not repeat the bits"
    dz = float(np.abs(z - r64["z"]).max())
    print(f"refineNoise [{mode}]: max |z - z64| = {dz:.3e} (bar {rp.NOISE_TOL:g}); loss {first.mean():.3e} -> {best.mean():.3e}")
    assert dz <= rp.NOISE_TOL
    assert np.abs(first - r64["first"]).max() <= 1e-4 * r64["first"].max() and np.abs(best - r64["best"]).max() <= 1e-4 * r64["first"].max()
    f4, b4, z4 = _refine(ctx, G, li, 4)                                            # chunks of 4 and 2 rows
    assert float(np.abs(z4 - r64["z"]).max()) <= rp.NOISE_TOL and float(np.abs(z4 - z).max()) <= rp.NOISE_TOL
    # G is what it was (mode, flag and counters: _refine): an ordinary forward in either mode gives the bits it gave
    G.evaluate(); assert np.array_equal(G.forward(probe), eval_before)
    G.training(); assert np.array_equal(G.forward(probe), train_before)
    assert TOL == rp.NOISE_TOL


def test_update_grad_input_of_a_compiled_model(ctx):
    """nn.Module:updateGradInput on host arrays: evaluate() only, and flag and forward counter are what they were afterwards"""
    from ganrev import nn, synth
    import ganrev._lib as L
    case = rp.BY_NAME["B-conv-sbn-elu-max"]
    d = rp.case_data(case.name)
    ctx.set_conv_mode("f32")
    m = nn.Sequential()
    m.add(nn.SpatialConvolution(4, 8, 3, 3, 1, 1, 1, 1)); m.add(nn.SpatialBatchNormalization(8)); m.add(nn.ELU()); m.add(nn.SpatialMaxPooling(2, 2))
    m.evaluate()
    m.forward(d["x"])
    m._net.set_params(d["params"])
    m._net.set_bn_running(0, *d["running"][0])
    out = m.forward(d["x"]).copy()
    counter = m._net.forward_counter()
    gin = m.updateGradInput(d["x"], d["gout"])
    assert m._net.forward_counter() == counter and not m._net.input_grad
    assert np.abs(gin.astype(np.float64) - d["ref"]["gin"]).max() <= rp.GRAD_RTOL * np.abs(d["ref"]["gin"]).max()
    assert np.array_equal(m.forward(d["x"]), out)
    m.training()
    m.forward(d["x"])
    with pytest.raises(L.GanrevError, match="evaluate"):
        m.updateGradInput(d["x"], d["gout"])


# ---------------------------------------------------------------------------------------------------------------- G
def test_refusals(ctx):
    import ganrev._lib as L
    case = rp.BY_NAME["B-linear-bn-relu"]
    d = rp.case_data(case.name)
    net = _make_net(ctx, case, d)
    try:
        with _Dev(ctx, d["x"], d["gout"]) as dev:
            net.forward_dev(dev.x, case.B)                                         # evaluate(), flag off
            with pytest.raises(L.GanrevError, match="GR_ERR_STATE.*gr_net_set_input_grad"):
                net.backward_input_dev(dev.x, dev.g, case.B, dev.gin)
            net.set_input_grad(True)
            with pytest.raises(L.GanrevError, match="GR_ERR_STATE.*gr_net_set_input_grad"):      # the flag alone is not a forward
                net.backward_input_dev(dev.x, dev.g, case.B, dev.gin)
            net.forward_dev(dev.x, case.B)
            with pytest.raises(L.GanrevError, match="GR_ERR_STATE.*batch 2 does not match"):
                net.backward_input_dev(dev.x, dev.g, 2, dev.gin)
            net.set_training(True)
            with pytest.raises(L.GanrevError, match="GR_ERR_STATE.*training mode"):
                net.backward_input_dev(dev.x, dev.g, case.B, dev.gin)
            net.forward_dev(dev.x, case.B)                                         # a training-mode forward with the flag on keeps nothing either
            net.set_training(False)
            with pytest.raises(L.GanrevError, match="GR_ERR_STATE.*gr_net_set_input_grad"):
                net.backward_input_dev(dev.x, dev.g, case.B, dev.gin)
            net.forward_dev(dev.x, case.B)
            net.backward_input_dev(dev.x, dev.g, case.B, dev.gin)                  # and now it runs
            with pytest.raises(L.GanrevError, match="GR_ERR_STATE.*requires training mode"):     # as before
                net.backward_dev(dev.x, dev.g, case.B, dev.gin)
    finally:
        net.close()


def _apply_r(tmp_path, name, extra):
    from ganrev import apply_r
    out = tmp_path / name
    apply_r.main(["--synthetic", "1x16x16x8", "--nbImages", "40", "--batchSize", "16", "--quiet", "--writeTo", str(out)] + extra)
    arrays = {f: np.load(out / f) for f in sorted(os.listdir(out)) if f.endswith(".npy")}
    summary = json.load(open(out / "summary.json"))
    return arrays, summary


def test_apply_r_refine_on_both_routes(ctx, tmp_path):
    from ganrev import apply_r
    plain, s_plain = _apply_r(tmp_path, "plain", [])
    zero, s_zero = _apply_r(tmp_path, "zero", ["--refine", "0"])
    assert plain.keys() == zero.keys() and all(plain[k].tobytes() == zero[k].tobytes() for k in plain), "--refine 0 changed an output"
    drop = lambda s: {k: v for k, v in s.items() if k != "embed_and_search_seconds"}
    assert drop(s_plain) == drop(s_zero) and "refine" not in s_zero
    dev, s_dev = _apply_r(tmp_path, "dev", ["--refine", "3", "--render"])
    assert os.path.getsize(tmp_path / "dev" / "refined_pairs.png") > 0 and not os.path.exists(tmp_path / "plain" / "refined_pairs.png")
    res, s_res = _apply_r(tmp_path, "res", ["--refine", "3", "--resident"])
    r = s_dev["refine"]
    assert r["steps"] == 3 and r["lr"] == 0.01 and r["loss_after_mean"] <= r["loss_before_mean"] and 0 <= r["rows_improved"] <= 40
    assert s_res["refine"] == r
    assert dev["attributes.npy"].tobytes() == res["attributes.npy"].tobytes(), "the two routes refine to different bits"
    assert dev["attributes_fixer.npy"].tobytes() == plain["attributes_fixer.npy"].tobytes(), "attributesFixer is left as R produced it"
    assert r["rows_improved"] > 0 and not np.array_equal(dev["attributes.npy"], plain["attributes.npy"])
    with pytest.raises(SystemExit):
        apply_r.parse(["--host", "--refine", "3"])
