"""GPU: models.create_G4 (reference models.lua:145-194) and what it is compiled to.

1. the grouped layer kinds alone (csrc/group.hip: GR_GROUPLINEAR, GR_GROUPCONV3, GR_PRELU with n >= 2 slopes) against float64 PyTorch
   (g4_oracle.torch_reference);
2. a miniature G4 as a bundle (one grouped gr_net, nn.bundle_plan) and on the parts route (`concat.bundle = False`: nb branch nets and a
   tail net, joined by nn.Concat(2) on the host or by device.DeviceModel on the device) against the CPU oracle, which never sees a grouped
   kind (g4_oracle.G4Oracle: one oracle net per branch and for the tail, joined in numpy), and against each other;
3. the full create_G4((1, 32, 32), 32);  4. the scripts.
All three convolution arithmetics wherever a 3x3 tail convolution runs; the grouped kinds are exact fp32 in each.

The project's bars: outputs within helpers.TOL = 1e-4 absolute, gradInput within 1e-4 of its largest entry, parameter gradients by
helpers.assert_grads_close(..., 1e-4, 1e-3) (g4_oracle.assert_segments_close: the same rule on a bare layer list).  A pre-activation
within rounding of zero flips the nn.PReLU derivative, so every case that compares gradients takes the first input seed of
g4_oracle.SEEDS (1..40) whose reference forward keeps every PReLU input 1e-4 away from zero.  At the full model size (B * 32 * (16 + 4096
+ 16384) + B * 65536 PReLU inputs) no such seed exists: that case compares forwards only."""
import numpy as np
import pytest

import ganrev._lib as L
from ganrev import adversarial, device, models, nn, nn_utils, synth, t7
from g4_oracle import G4Oracle, KINK_GAP, SEEDS, assert_segments_close, mini_g4, pick_seed, torch_reference
from helpers import TOL, assert_close, assert_grads_close

pytestmark = pytest.mark.gpu

GROUP_KERNELS = {"grouplinear": {"grouplinear_forward_kernel", "grouplinear_dgrad_kernel", "grouplinear_wgrad_kernel"},
                 "groupconv3": {"groupconv3_forward_kernel", "groupconv3_dgrad_kernel", "groupconv3_wgrad_kernel", "group_wgrad_reduce_kernel"},
                 "prelu_multi": {"prelu_multi_forward_kernel", "prelu_multi_backward_kernel", "prelu_multi_grad_kernel"}}


# ---------------------------------------------------------------------------------------------------------------- 1. the kinds alone
def _layer_list_vs_torch(ctx, descs, dims, B, what, kernels=()):
    """A bare layer list as one gr_net: forward, gradInput and every parameter gradient against float64 PyTorch; a second backward
    without zero_grads doubles the gradients exactly (+=); a second run gives the same bits; the named kernels ran."""
    net = L.Net(ctx, descs, dims)
    try:
        theta = synth.uniform((net.n_params,), 3, -0.5, 0.5)
        net.set_params(theta)
        net.set_training(True)
        shape = (B,) + L.Net._shape(dims)
        has_prelu = any(d[0] == L.PRELU for d in descs)
        for seed in SEEDS:                      # (without a PReLU the first seed is taken)
            x = synth.normal(shape, seed)
            gout = synth.normal((B,) + L.Net._shape(net.out_dims), seed + 100)
            ref = torch_reference(descs, dims, theta, x, gout)
            if not has_prelu or ref["kink"] >= KINK_GAP:
                break
        else:
            raise AssertionError(f"{what}: no input seed keeps every PReLU input {KINK_GAP:g} away from zero")
        ctx.set_timing(2)
        out = net.forward(x).copy()
        net.zero_grads()
        gin = net.backward(x, gout).copy()
        names = {k["kernel"] for k in ctx.kernel_times()}
        ctx.set_timing(0)
        g1 = net.get_grads()
        assert set(kernels) <= names, sorted(names)
        d_out = float(np.abs(out - ref["out"].reshape(out.shape)).max())
        gmax = float(np.abs(ref["gin"]).max())
        d_gin = float(np.abs(gin - ref["gin"]).max()) / gmax
        print(f"[{what}] input seed {seed}: out {d_out:.2e}  gin {d_gin:.2e} (relative to max |gin| {gmax:.3g})")
        assert d_out <= TOL and d_gin <= TOL
        assert_segments_close(g1, ref["grads"], ref["segs"], what)
        net.backward(x, gout)
        g2 = net.get_grads()
        assert np.array_equal(g2, g1 + g1), float(np.abs(g2 - 2 * g1).max())
        out_b = net.forward(x)
        net.zero_grads()
        gin_b = net.backward(x, gout)
        assert np.array_equal(out_b, out) and np.array_equal(gin_b, gin) and np.array_equal(net.get_grads(), g1)
    finally:
        ctx.set_timing(0)
        net.close()


# B, a, b, G: nothing aligned, three groups | one group, one row | create_G4's own instance
@pytest.mark.parametrize("B,a,b,G", [(3, 15, 21, 3), (1, 5, 7, 1), (2, 512, 131072, 32)])
def test_grouplinear_alone(ctx, B, a, b, G):
    _layer_list_vs_torch(ctx, [(L.GROUPLINEAR, a, b, G, 0.0, 0)], (a, 1, 1), B, f"GROUPLINEAR {a}->{b} G={G} B={B}", GROUP_KERNELS["grouplinear"])


# B, a, b, G, H, W (the convolution's planes), up: 2 -> 3 planes per group on 5x7 | the same behind an up-sampling 3x4 -> 6x8 | G4's own
@pytest.mark.parametrize("B,a,b,G,H,W,up", [(3, 6, 9, 3, 5, 7, False), (3, 6, 9, 3, 6, 8, True), (2, 512, 512, 32, 32, 32, True)])
def test_groupconv3_alone(ctx, B, a, b, G, H, W, up):
    descs = ([(L.UPSAMPLE2, 0, 0, 0, 0.0, 0)] if up else []) + [(L.GROUPCONV3, a, b, G, 0.0, 0)]
    dims = (a, H // 2, W // 2) if up else (a, H, W)
    _layer_list_vs_torch(ctx, descs, dims, B, f"GROUPCONV3 {a}->{b} G={G} {H}x{W}{' up' if up else ''} B={B}", GROUP_KERNELS["groupconv3"])


PRELU_CASES = {
    "n=3 over C=6 at 5x7": ([(L.PRELU, 3, 0, 0, 0.0, 0)], (6, 5, 7)),
    "n=C": ([(L.PRELU, 6, 0, 0, 0.0, 0)], (6, 5, 7)),
    "behind a Linear": ([(L.LINEAR, 5, 6, 0, 0.0, 0), (L.PRELU, 3, 0, 0, 0.0, 0)], (5, 1, 1)),
    "behind a BatchNorm": ([(L.LINEAR, 5, 6, 0, 0.0, 0), (L.BN, 6, 0, 0, 0.0, 0), (L.PRELU, 3, 0, 0, 0.0, 0)], (5, 1, 1)),
    "behind conv + BatchNorm": ([(L.CONV3, 2, 6, 0, 0.0, 0), (L.BN, 6, 0, 0, 0.0, 0), (L.PRELU, 3, 0, 0, 0.0, 0)], (2, 5, 7)),
    "behind a grouped conv + BatchNorm": ([(L.GROUPCONV3, 4, 6, 2, 0.0, 0), (L.BN, 6, 0, 0, 0.0, 0), (L.PRELU, 2, 0, 0, 0.0, 0), (L.CONV3, 6, 2, 0, 0.0, 0)], (4, 5, 7)),
}


@pytest.mark.parametrize("case", sorted(PRELU_CASES))
def test_multi_slope_prelu(ctx, conv_mode, case):
    descs, dims = PRELU_CASES[case]
    _layer_list_vs_torch(ctx, descs, dims, 3, f"PReLU {case} {conv_mode}", GROUP_KERNELS["prelu_multi"])


def test_one_slope_prelu_is_todays_layer(ctx):
    """a = 0 and a = 1 are the shared slope, bit for bit: the same stage, the same kernels"""
    x, gout = synth.normal((3, 6, 5, 7), 1), synth.normal((3, 6, 5, 7), 2)
    res = []
    for a in (0, 1):
        net = L.Net(ctx, [(L.CONV3, 6, 6, 0, 0.0, 0), (L.PRELU, a, 0, 0, 0.0, 0)], (6, 5, 7))
        net.set_params(synth.uniform((net.n_params,), 3, -0.3, 0.3))
        ctx.set_timing(2)
        out = net.forward(x).copy(); net.zero_grads(); gin = net.backward(x, gout).copy()
        names = {k["kernel"] for k in ctx.kernel_times()}
        ctx.set_timing(0)
        assert not (names & GROUP_KERNELS["prelu_multi"]) and "prelu_grad_kernel" in names, sorted(names)
        res.append((net.n_params, out, gin, net.get_grads()))
        net.close()
    assert res[0][0] == res[1][0] and all(np.array_equal(p, q) for p, q in zip(res[0][1:], res[1][1:]))


@pytest.mark.parametrize("descs,dims,word", [
    ([(L.GROUPLINEAR, 15, 21, 2, 0.0, 0)], (15, 1, 1), "layer 0: grouped linear 15 -> 21 does not divide into 2 groups"),
    ([(L.GROUPLINEAR, 15, 21, 0, 0.0, 0)], (15, 1, 1), "layer 0: grouped linear 15 -> 21 does not divide into 0 groups"),
    ([(L.GROUPLINEAR, 12, 21, 3, 0.0, 0)], (15, 1, 1), "layer 0: grouped linear expects 12 inputs, got 15"),
    ([(L.GROUPCONV3, 6, 9, 2, 0.0, 0)], (6, 5, 7), "layer 0: grouped conv 6 -> 9 does not divide into 2 groups"),
    ([(L.GROUPCONV3, 6, 9, 3, 0.0, 0)], (3, 5, 7), "layer 0: grouped conv expects 6 input planes, got 3"),
    ([(L.LINEAR, 5, 6, 0, 0.0, 0), (L.PRELU, 4, 0, 0, 0.0, 0)], (5, 1, 1), "layer 1: PReLU with 4 slopes does not divide 6 channels"),
])
def test_bad_divisibility_is_refused_by_name(ctx, descs, dims, word):
    with pytest.raises(L.GanrevError) as e:
        L.Net(ctx, descs, dims)
    assert "GR_ERR_INVALID" in str(e.value) and word in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------- 2. the miniature
ND, B = 5, 3
_SEED = {}


def _mini_input(oracle):
    """the input seed of the miniature's gradient cases, chosen once on the CPU (the oracle is exact fp32 whatever the device's mode)"""
    if "mini" not in _SEED:
        seed, _, _ = pick_seed(G4Oracle(oracle, mini_g4(bundle=False), (ND, 1, 1)), (B, ND), True)
        _SEED["mini"] = seed
    return _SEED["mini"], synth.normal((B, ND), _SEED["mini"])


@pytest.mark.parametrize("route", ["bundle", "parts"])
def test_miniature_vs_oracle(oracle, conv_mode, route):
    """nb = 3 branches of Linear(5, 4) - PReLU - Linear(4, 32) - BN - PReLU - Reshape(2, 4, 4) - up-sampling - conv 2 -> 2 - BN - PReLU, tail
    conv 6 -> 4 - BN - PReLU - conv 4 -> 1 - Sigmoid, B = 3: training forward, gradInput, every parameter gradient in getParameters()
    order; the running statistics of all 2 * 3 + 1 BatchNorm modules after that forward; the evaluate() forward with them."""
    seed, x = _mini_input(oracle)
    model = mini_g4(bundle=route == "bundle")
    og = G4Oracle(oracle, mini_g4(bundle=False), (ND, 1, 1))
    if route == "bundle":
        assert model.children() is None and len(model._param_chunks()) == 1
    else:
        assert [type(p).__name__ for p in model.parts()] == ["Concat", "Sequential"] and len(model._param_chunks()) == 4
    flat, grads = model.getParameters()
    assert np.array_equal(og.params, flat)
    model.training(); og.set_training(True)
    ref = og.forward(x)
    gap = og.min_kink_distance()
    out = model.forward(x)
    print(f"[mini G4 {route} {conv_mode}] input seed {seed}: smallest |PReLU input| {gap:.2e}, out {float(np.abs(out - ref).max()):.2e}")
    assert gap >= KINK_GAP and out.shape == (B, 1, 8, 8)
    assert_close(out, ref, TOL, "training forward")
    gy = synth.normal(ref.shape, 9)
    grads[...] = 0; og.zero_grads()
    gin = model.backward(x, gy)
    ref_gin = og.backward(x, gy)
    assert gin.shape == x.shape
    assert_close(gin, ref_gin, TOL * float(np.abs(ref_gin).max()), "gradInput")
    assert_grads_close(model, grads, og.grads, 1e-4, 1e-3, f"mini G4 {route}")
    model.pull_params()
    assert np.array_equal(flat, og.params)                     # a pull brings back what was pushed, in tree order
    stats = og.bn_running()
    bns = [m for m in model.leaves() if hasattr(m, "running_mean")]
    assert len(stats) == len(bns) == 7
    for m, (_, rm, rv) in zip(bns, stats):
        assert_close(m.running_mean, rm, TOL, f"{m.typename} running_mean"); assert_close(m.running_var, rv, TOL, f"{m.typename} running_var")
    model.evaluate(); og.set_training(False)
    assert_close(model.forward(x), og.forward(x), TOL, "evaluate() forward")


def test_miniature_bundle_adam_step_and_determinism(oracle, ctx, conv_mode):
    """One fused Adam step on the bundle's one net, then pull, against the oracle's step in tree order on the same gradient (the bit-exact
    rule gr_adam_step is held to: penalty, clamp and Adam are element-wise, so the net's layer-major order cannot show); Adam's moments
    come back in tree order too.  Two runs of the bundle give the same bits."""
    _, x = _mini_input(oracle)
    gy = synth.normal((B, 1, 8, 8), 9)
    runs = []
    for _ in range(2):
        model = mini_g4()
        model.training()
        flat, grads = model.getParameters()
        theta0 = flat.copy()
        out = model.forward(x).copy()
        grads[...] = 0
        gin = model.backward(x, gy).copy()
        net = model._net
        assert np.array_equal(net.get_grads(), grads) and np.array_equal(net.get_params(), theta0)
        net.adam_reset()
        hyper = dict(l1=1e-4, l2=1e-3, clamp=5.0)
        net.adam_step(L.Hyper(**hyper), 1)
        theta, g, m, v = theta0.copy(), grads.copy(), np.zeros_like(theta0), np.zeros_like(theta0)
        oracle.penalty_clamp_adam(theta, g, m, v, oracle.GoHyper(**hyper), 1)
        model._flat = None                                   # the modules take what the device holds
        model.pull_params()
        assert np.array_equal(model._flat_host(), theta)
        dm, dv = net.adam_state()
        assert np.array_equal(dm, m) and np.array_equal(dv, v)
        runs.append((out, gin, grads.copy(), theta))
    assert all(np.array_equal(p, q) for p, q in zip(*runs))


def test_miniature_bundle_vs_parts_on_the_device(ctx, oracle, conv_mode):
    """the same model as one grouped net and as nb + 1 nets inside device.DeviceModel: same parameters, same input, within the bars"""
    _, x = _mini_input(oracle)
    gy = synth.normal((B, 1, 8, 8), 9)
    res = {}
    for route in ("bundle", "parts"):
        model = mini_g4(bundle=route == "bundle")
        model.training()
        model.forward(x)                                     # compile
        dm = device.DeviceModel(ctx, model)
        xd, gd = ctx.upload(x), ctx.upload(gy)
        try:
            assert len(dm.nets) == (1 if route == "bundle" else 4)
            dm.set_training(True); dm.zero_grads()
            out = ctx.download(dm.forward(xd, B), (B, 1, 8, 8))
            gin = ctx.download(dm.backward(gd, B, True), x.shape)
            res[route] = (model, out, gin, np.concatenate([n.get_grads() for n in dm.nets]))
        finally:
            ctx.free(xd); ctx.free(gd); dm.close()
    (_, out_b, gin_b, g_b), (parts, out_p, gin_p, g_p) = res["bundle"], res["parts"]
    assert_close(out_b, out_p, TOL, "forward")
    assert_close(gin_b, gin_p, TOL * float(np.abs(gin_p).max()), "gradInput")
    assert_grads_close(parts, g_b, g_p, 1e-4, 1e-3, "bundle vs parts")


def _flat_dev(dm, what):
    return np.concatenate([getattr(n, what)() for n in dm.nets])


def test_miniature_on_device_model_equals_host_containers(oracle, ctx, conv_mode):
    """The parts route: device.DeviceModel on [B x C x H x W] branch outputs.  Joining channels in NCHW is joining each sample's features, so
    forward, gradInput and the flat gradient are those of the host containers bit for bit (the same nets run the same kernels, the
    gradInput sum is the same float32 additions in branch order).  Twice, with nothing allocated in the second step.  Then one fused Adam
    step per part against the oracle's step on the flat vectors in tree order."""
    _, x = _mini_input(oracle)
    model = mini_g4(bundle=False)
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
        assert len(dm.nets) == 4 and dm.out_dims(model) == (1, 8, 8) and dm.out_dims(model.parts()[0]) == (6, 8, 8)
        dm.set_training(True)
        for _ in range(2):
            dm.zero_grads()
            out_d = ctx.download(dm.forward(xd, B), out.shape)
            gin_d = ctx.download(dm.backward(gd, B, True), x.shape)
            assert np.array_equal(out_d, out), float(np.abs(out_d - out).max())
            assert np.array_equal(gin_d, gin), float(np.abs(gin_d - gin).max())
            assert np.array_equal(_flat_dev(dm, "get_grads"), g_host)
        live = dict(dm.mem.nbytes)
        dm.forward(xd, B); dm.backward(gd, B, True)
        assert dm.mem.nbytes == live
        theta = _flat_dev(dm, "get_params")
        assert np.array_equal(theta, flat)
        dm.adam_reset()
        dm.zero_grads(); dm.forward(xd, B); dm.backward(gd, B, False)
        dm.adam_step(L.Hyper(l1=0.0, l2=0.0, clamp=5.0), 1)
        m, v = np.zeros_like(theta), np.zeros_like(theta)
        oracle.penalty_clamp_adam(theta, g_host.copy(), m, v, oracle.GoHyper(l1=0.0, l2=0.0, clamp=5.0), 1)
        assert np.array_equal(_flat_dev(dm, "get_params"), theta)
    finally:
        ctx.free(xd); ctx.free(gd); dm.close()


def test_device_model_refuses_branches_that_do_not_line_up(ctx):
    model = nn.Sequential()
    cat = nn.Concat(2)
    cat.add(nn.Sequential().add(nn.Linear(4, 8)).add(nn.Reshape(2, 2, 2)))
    cat.add(nn.Sequential().add(nn.Linear(4, 8)).add(nn.Reshape(2, 4, 1)))
    model.add(cat)
    assert model.children() is not None                   # (unequal branches: no bundle)
    for b in cat.modules:
        b.forward(synth.normal((2, 4), 1))                 # the host nn.Concat itself refuses the pair, so each branch is compiled on its own
    with pytest.raises(L.GanrevError, match="do not line up"):
        device.DeviceModel(ctx, model)
    with pytest.raises(L.GanrevError, match="do not line up"):
        model.forward(synth.normal((2, 4), 1))
    other = nn.Sequential().add(nn.Concat(1).add(nn.Linear(4, 8)))
    other.forward(synth.normal((2, 4), 1))
    with pytest.raises(L.GanrevError, match=r"only nn.Concat\(2\)"):
        device.DeviceModel(ctx, other)


# ---------------------------------------------------------------------------------------------------------------- 3. the full model
FULL_DIMS, FULL_ND, FULL_B = (1, 32, 32), 32, 4
_FULL = {}


def _full_model(bundle=True):
    G = synth.init_params(models.create_G4(FULL_DIMS, FULL_ND, seed=6), 7)
    if not bundle:
        G.modules[1].bundle = False
    return G


def _full_reference(oracle):
    """the oracle's training and evaluate() forwards of create_G4((1, 32, 32), 32) at B = 4, computed once for every case and arithmetic"""
    if not _FULL:
        og = G4Oracle(oracle, _full_model(False), (FULL_ND, 1, 1))
        x = synth.normal((FULL_B, FULL_ND), 8)
        og.set_training(True)
        _FULL["train"] = og.forward(x)
        og.set_training(False)
        _FULL["eval"] = og.forward(x)
        _FULL["stats"] = [(rm, rv) for _, rm, rv in og.bn_running()]
        _FULL["x"] = x
    return _FULL


@pytest.mark.parametrize("route", ["bundle", "parts"])
def test_full_model_forward_vs_oracle(oracle, conv_mode, route):
    ref = _full_reference(oracle)
    G = _full_model(route == "bundle")
    assert len(G._param_chunks()) == (1 if route == "bundle" else 33) and (G.children() is None) == (route == "bundle")
    G.training()
    out = G.forward(ref["x"])
    assert out.shape == (FULL_B,) + FULL_DIMS
    print(f"[create_G4 {route} {conv_mode}] training forward {float(np.abs(out - ref['train']).max()):.2e}")
    assert_close(out, ref["train"], TOL, "training forward")
    G.pull_params()
    bns = [m for m in G.leaves() if hasattr(m, "running_mean")]
    assert len(bns) == 65
    for m, (rm, rv) in zip(bns, ref["stats"]):
        assert_close(m.running_mean, rm, TOL, "running_mean"); assert_close(m.running_var, rv, TOL, "running_var")
    G.evaluate()
    out = G.forward(ref["x"])
    print(f"[create_G4 {route} {conv_mode}] evaluate() forward {float(np.abs(out - ref['eval']).max()):.2e}")
    assert_close(out, ref["eval"], TOL, "evaluate() forward")


def test_full_model_on_the_resident_paths(ctx, conv_mode):
    """The bundle is a plain net to nn_utils.forwardBatchedDev and apply_r.embed_dev: ragged chunks (4, 4, 2 rows) give, bit for bit, what
    forward gives chunk by chunk (same kernels, same chunking) and, within the bar, what one forward of all rows gives; embed_dev with a
    small R leaves what the host loop leaves."""
    from ganrev import apply_r
    G = _full_model()
    G.evaluate()
    N, chunk = 10, 4
    noise = synth.normal((N, FULL_ND), 12)
    whole = G.forward(noise).copy()
    by_chunk = np.concatenate([G.forward(noise[lo:lo + chunk]).copy() for lo in range(0, N, chunk)])
    dn = nn_utils.DeviceTensor(ctx, noise.shape)
    ctx.upload(noise, dn.ptr)
    out = nn_utils.forwardBatchedDev(G, dn, chunk)
    got = out.numpy()
    assert G.children() is None and np.array_equal(got, by_chunk)
    assert_close(got, whole, TOL, "ragged chunks vs one forward")
    R = synth.init_params(models.create_R(FULL_DIMS, FULL_ND, seed=2), 3)
    images, attrs = apply_r.embed_dev(G, R, dn, chunk, keep_images=True)
    h_images, h_attrs = apply_r.embed(G, R, noise, chunk)
    assert np.array_equal(images.numpy(), h_images) and np.array_equal(attrs.numpy(), h_attrs)
    for t in (dn, out, images, attrs):
        t.free()


@pytest.mark.parametrize("route", ["bundle", "parts"])
def test_device_game_trains_the_full_model(ctx, route):
    """adversarial.DeviceGame with create_G4 against create_D2, G as one grouped net or as 33 nets inside device.DeviceModel.  One batch with
    given noise: the losses are finite, every parameter tensor's share of the flat vector took its Adam step and every BatchNorm of G moved
    its running statistics."""
    Bg = 4
    G, D = models.create_G4(FULL_DIMS, FULL_ND, True, 3), models.create_D2(FULL_DIMS, True, 4)
    if route == "parts":
        G.modules[1].bundle = False
    env = adversarial.make_env(G, D, FULL_DIMS, batchSize=Bg, noiseDim=FULL_ND, N_epoch=1)
    game = adversarial.DeviceGame(env)
    try:
        assert len(game.gg.nets) == (1 if route == "bundle" else 33)
        before = env.PARAMETERS_G.copy()
        noise_d, noise_g = synth.normal((Bg // 2, FULL_ND), 21), synth.normal((Bg, FULL_ND), 22)
        loss_d, loss_g = game.batch(synth.uniform((Bg // 2,) + FULL_DIMS, 23, 0, 1), noise_d=noise_d, noise_g=noise_g, want_loss=True)
        assert np.isfinite(loss_d) and np.isfinite(loss_g) and loss_d > 0 and loss_g > 0
        game.sync_to_host()
        assert np.all(np.isfinite(env.PARAMETERS_G))
        off = 0
        for m in G.leaves():
            for a in m.param_arrays():
                assert not np.array_equal(env.PARAMETERS_G[off:off + a.size], before[off:off + a.size]), f"{m.typename} [{off}:{off + a.size}] did not move"
                off += a.size
        assert all(m.running_mean.any() for m in G.leaves() if hasattr(m, "running_mean"))
    finally:
        game.close()


# ---------------------------------------------------------------------------------------------------------------- 4. scripts
def test_scripts_carry_a_g4_checkpoint(tmp_path):
    """ganrev.train --G_model create_G4 writes a checkpoint that loads back as the same tree and compiles to one net; train_r's
    device-resident loop and apply_r's device-resident pipeline run on it unchanged; any other image size is refused."""
    from ganrev import apply_r, train, train_r
    nd = 8
    res = train.main(["--G_model", "create_G4", "--epochs", "1", "--N_epoch", "2", "--batchSize", "4", "--noiseDim", str(nd), "--colorSpace", "y", "--save", str(tmp_path / "gan"), "--quiet"])
    ck = t7.load_checkpoint(res["path"])
    G = ck["G"]
    assert "_unconverted" not in ck and G.children() is None and np.all(np.isfinite(res["last_losses"]))
    assert [m.typename for m in G.modules[0].modules[0].modules][5] == "nn.Reshape"
    assert np.array_equal(G._flat_host(), res["env"].MODEL_G._flat_host())
    common = ["--G", res["path"], "--nbBatches", "2", "--batchSize", "4", "--quiet"]
    _, R, losses = train_r.main(common + ["--save", str(tmp_path / "r.net")])
    assert len(losses) == 2 and np.all(np.isfinite(losses))
    train_r.main(common + ["--fixer", "--save", str(tmp_path / "r_fixer.net")])
    summary = apply_r.main(["--G", res["path"], "--R", str(tmp_path / "r.net"), "--R_fixer", str(tmp_path / "r_fixer.net"),
                            "--nbImages", "64", "--batchSize", "8", "--writeTo", str(tmp_path / "out"), "--quiet"])
    assert summary["path"] == "device" and summary["dims"] == [1, 32, 32] and summary["noiseDim"] == nd
    assert np.load(tmp_path / "out" / "variations.npy").shape == (nd, 16, 1, 32, 32) and np.load(tmp_path / "out" / "attributes.npy").shape == (64, nd)
    with pytest.raises(SystemExit, match="create_G4 paints 32x32 images only"):
        train.main(["--G_model", "create_G4", "--height", "64", "--epochs", "1", "--N_epoch", "1", "--batchSize", "4", "--quiet"])
