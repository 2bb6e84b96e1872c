"""GPU: penalty + clamp + optim.sgd | adagrad | adadelta | adamax | rmsprop as one fused launch (gr_optim_step, csrc/elem.hip) against the chain it
replaces - adversarial.penalise_and_clamp followed by the float32 mirror of the rock in ganrev/optim.py - BIT FOR BIT, and the device-resident GAN game
(adversarial.DeviceGame) dispatching it for D and for G.

Why bit-exact can be asked (it is the bar gr_adam_step is held to): both sides are IEEE float32 add / mul / div / sqrt in one order, the library is
compiled without contraction, and every scalar is rounded to float32 once from the same double expression."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ["sgd", "adagrad", "adadelta", "adamax", "rmsprop"]
# the config table each case hands to the mirror and, through L.OptimConfig, to the device: the five methods on the rock's defaults (an empty
# table), and sgd with every option it carries - momentum 0 and 0.5 (dampening then defaults to the momentum), nesterov, weightDecay, learningRateDecay
CASES = {
    "sgd": ("sgd", {}),
    "adagrad": ("adagrad", {}),
    "adadelta": ("adadelta", {}),
    "adamax": ("adamax", {}),
    "rmsprop": ("rmsprop", {}),
    "sgd-momentum0": ("sgd", {"learningRate": 0.02, "momentum": 0.0, "weightDecay": 1e-3, "learningRateDecay": 0.1}),
    "sgd-momentum0.5": ("sgd", {"learningRate": 0.02, "momentum": 0.5}),
    "sgd-nesterov": ("sgd", {"learningRate": 0.02, "momentum": 0.5, "dampening": 0.0, "nesterov": True, "weightDecay": 1e-3, "learningRateDecay": 0.1}),
}
L2_CLAMP = dict(l1=0.0, l2=1e-4, clamp=1.0)
L1_CLAMP = dict(l1=1e-3, l2=0.0, clamp=1.0)      # (with both penalties non-zero the mirror sums them in another association than the kernels: not a case)
# nn.Linear nets: 3 parameters = the tail alone; 18 = four 16-byte vectors + a tail of two; 4 198 401 > 4096 blocks x 256 threads x 4 entries, so the
# grid-stride loop wraps, and the count is odd
SIZES = {3: (2, 1), 18: (5, 3), 4198401: (2048, 2049)}
SENTINEL = np.float32(1234.5)
SPECIALS = np.array([0.0, 0.0, 1e-30, -1e-30, 3.0, -3.0], np.float32)      # exact zeros, far below sqrt(FLT_MIN), beyond the clamp


@functools.lru_cache(maxsize=None)
def _net(n):
    from ganrev import nn, synth
    fin, fout = SIZES[n]
    lin = nn.Linear(fin, fout)
    lin.forward(synth.normal((1, fin), 3))
    assert lin._net.n_params == n
    return lin                                               # (the module owns its net)


@functools.lru_cache(maxsize=None)
def _vectors(n):
    """(parameters, the three steps' gradients) for a net of n parameters, computed once and never written to"""
    from ganrev import synth
    theta = synth.normal((n,), 4) * np.float32(0.05)
    theta[n // 2] = 0.0                                      # sign(0) = 0 in the L1 penalty
    grads = []
    for step in range(3):
        g = synth.normal((n,), 7 + step) * np.float32(0.7)
        if n < SPECIALS.size:
            if step < 2:
                g[:] = SPECIALS[3 * step:3 * step + 3]     # step 1: (0, 0, 1e-30), step 2: (-1e-30, 3, -3), step 3: ordinary values
        else:
            where = np.array([0, 1, n // 3, n // 2, n - 2, n - 1])      # the first vector, the middle, the tail
            g[where] = np.roll(SPECIALS, step)            # step 1 has its zeros at entries 0 and 1: adamax divides 0 by u = 0 + 1e-38 there
        g.setflags(write=False)
        grads.append(g)
    theta.setflags(write=False)
    return theta, grads


def _mirror_step(method, theta, g, state, pen):
    """the host chain of one batch: adversarial.lua:86-88 then optim[method] on copies -> the penalised, clamped gradient"""
    from ganrev import adversarial, optim
    g = g.copy()
    adversarial.penalise_and_clamp(theta, g, 0.0, pen["l1"], pen["l2"], pen["clamp"])
    kept = g.copy()
    optim.METHODS[method](lambda _: (0.0, g), theta, state)
    assert np.array_equal(g, kept)                           # the rule does not write the closure's gradient (sgd's weight decay goes to a clone)
    return g


def _check_state(L, method, cfg, state, slots, what):
    for key, used, got in zip(L.OPT_STATE_KEYS[method], cfg.slots(), slots):
        if used:
            assert np.array_equal(got, state[key]), f"{what}: state slot '{key}'"
        else:
            assert np.all(got == SENTINEL), f"{what}: a slot {method} does not use was written"


@pytest.mark.parametrize("n", sorted(SIZES))
@pytest.mark.parametrize("case,pen", [(c, L2_CLAMP) for c in CASES] + [("adadelta", L1_CLAMP)],
                         ids=list(CASES) + ["adadelta-l1"])
def test_optim_step_equals_the_host_mirror_bit_for_bit(case, pen, n):
    import ganrev._lib as L
    method, table = CASES[case]
    net = _net(n)._net
    theta0, grads = _vectors(n)
    cfg = L.OptimConfig(method, table, **pen)
    theta, state = theta0.copy(), dict(table)
    net.set_params(theta0)
    net.optim_reset()
    zero = net.optim_state()
    assert not zero[0].any() and not zero[1].any()
    fill = np.full(n, SENTINEL, np.float32)
    net.set_optim_state(*(None if used else fill for used in cfg.slots()))
    for step in range(3):
        net.set_grads(grads[step])
        net.optim_step(cfg, step + 1)
        want_g = _mirror_step(method, theta, grads[step], state, pen)
        assert np.all(np.isfinite(theta)), f"{case} step {step + 1}: the mirror itself left the finite numbers"
        what = f"{case}, {n} parameters, step {step + 1}"
        got = net.get_params()
        assert np.array_equal(got, theta), f"{what}: {(got != theta).sum()} parameters differ, first at {np.flatnonzero(got != theta)[:4]}"
        assert np.array_equal(net.get_grads(), want_g), f"{what}: stored gradient"
        _check_state(L, method, cfg, state, net.optim_state(), what)
    assert not np.array_equal(theta, theta0)


def test_optim_step_refusals_on_a_live_net_launch_nothing():
    import ganrev._lib as L
    net = _net(18)._net
    theta0, grads = _vectors(18)
    net.set_params(theta0); net.set_grads(grads[2]); net.optim_reset()
    for cfg, t, msg in ((L.OptimConfig(99), 1, "unknown optimizer method 99"), (L.OptimConfig(0), 1, "unknown optimizer method 0"),
                        (L.OptimConfig("sgd", {"nesterov": True}), 1, "Nesterov momentum requires a momentum and zero dampening"),
                        (L.OptimConfig("sgd", {"nesterov": True, "momentum": 0.5}), 1, "Nesterov momentum requires"),
                        (L.OptimConfig("sgd"), 0, "t = 0")):
        with pytest.raises(L.GanrevError, match=msg) as e:
            net.optim_step(cfg, t)
        assert "GR_ERR_INVALID" in str(e.value)
    a, b = net.optim_state()
    assert np.array_equal(net.get_params(), theta0) and np.array_equal(net.get_grads(), grads[2]) and not a.any() and not b.any()
    # the mirror refuses the same nesterov requests
    from ganrev import optim
    for table in ({"nesterov": True}, {"nesterov": True, "momentum": 0.5}):
        with pytest.raises(ValueError):
            optim.sgd(lambda x: (0.0, x), theta0.copy(), dict(table))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# adversarial.DeviceGame with --D_optmethod / --G_optmethod other than adam, at the shapes of test_adversarial_game_with_the_other_optimisers
DIMS, ND, B = (1, 16, 16), 8, 8


def _env(**opt):
    from ganrev import adversarial, models
    G, D = models.create_G(DIMS, ND, True, 3), models.create_D2(DIMS, True, 4)
    return adversarial.make_env(G, D, DIMS, batchSize=B, noiseDim=ND, N_epoch=1, seed=5, D_sgd_momentum=0.5, G_sgd_momentum=0.5, **opt)


def _flat(model, read):
    """read(net) of every compiled part joined in getParameters() order"""
    chunks = model._param_chunks()
    out = np.zeros(max(hi for _, _, hi in chunks), np.float32)
    for ch, lo, hi in chunks:
        if hi > lo:
            out[lo:hi] = read(ch._net)
    return out


@pytest.mark.parametrize("which", ["D", "G"])
@pytest.mark.parametrize("method", METHODS)
def test_device_game_first_step_is_the_mirrors_rule(method, which):
    """One update of one net from the empty state train.lua:183-193 gives it: the parameters after the batch equal the mirror's rule applied to
    the parameters before it and the penalised, clamped gradient the batch stored, bit for bit; the state is the mirror's."""
    import ganrev._lib as L
    from ganrev import adversarial, optim, synth
    env = _env(D_optmethod=method, G_optmethod=method, D_iterations=int(which == "D"), G_iterations=int(which == "G"))
    game = adversarial.DeviceGame(env)
    model = env.MODEL_D if which == "D" else env.MODEL_G
    other = env.MODEL_G if which == "D" else env.MODEL_D
    before, other_before = _flat(model, lambda n: n.get_params()), _flat(other, lambda n: n.get_params())
    game.batch(synth.uniform((B // 2,) + DIMS, 40, 0, 1))
    g = _flat(model, lambda n: n.get_grads())
    after = _flat(model, lambda n: n.get_params())
    clampv = env.OPT.D_clamp if which == "D" else env.OPT.G_clamp
    assert g.any() and np.abs(g).max() <= clampv
    state = dict(env.OPTSTATE[method][which])
    want = before.copy()
    optim.METHODS[method](lambda _: (0.0, g), want, state)
    assert np.array_equal(after, want), f"{method} {which}: {(after != want).sum()} of {want.size} parameters differ from the mirror's first step"
    assert not np.array_equal(after, before) and np.array_equal(_flat(other, lambda n: n.get_params()), other_before)      # 0 iterations: frozen
    cfg = game.hyper_d if which == "D" else game.hyper_g
    assert isinstance(cfg, L.OptimConfig) and cfg.method == L.OPT_METHODS[method]
    if method == "sgd":
        assert (cfg.learningRate, cfg.momentum, cfg.dampening) == (0.02, 0.5, 0.5)       # OPT.X_sgd_lr, OPT.X_sgd_momentum (train.lua:189-190)
    for slot, (key, used) in enumerate(zip(L.OPT_STATE_KEYS[method], cfg.slots())):
        got = _flat(model, lambda n: n.optim_state()[slot])
        assert np.array_equal(got, state[key]) if used else not got.any(), (method, which, key)
    game.close()


@pytest.mark.parametrize("method", METHODS)
def test_device_game_batch_hands_its_state_to_the_host_game(method):
    """One whole batch (D then G), then sync_to_host(): env.OPTSTATE[method] holds the device's state under the mirror's keys, adam's tables stay
    empty, adversarial.train continues from it.  D's first loss does not depend on the optimiser: it agrees with adversarial.train from the same
    state and noise within the 1e-5 relative bar of test_device_resident_gan_batch_matches_the_host_mirror.  The parameters after the batch are
    compared with the host game's and the figures PRINTED, not asserted: the host game's gradients come from other entry points and a normalised
    update amplifies their last bit (DESIGN.md section 0 records what this prints)."""
    import ganrev._lib as L
    from ganrev import adversarial, nn_utils, synth
    host, dev = _env(D_optmethod=method, G_optmethod=method), _env(D_optmethod=method, G_optmethod=method)
    assert np.array_equal(host.PARAMETERS_D, dev.PARAMETERS_D) and np.array_equal(host.PARAMETERS_G, dev.PARAMETERS_G)
    game = adversarial.DeviceGame(dev)
    host.MODEL_D.forward(host.MODEL_G.forward(nn_utils.createNoiseInputs(2, ND, "normal", seed=1)))      # the game's compile forward, mirrored
    real = synth.uniform((B // 2,) + DIMS, 40, 0, 1)
    noise_d = nn_utils.createNoiseInputs(B // 2, ND, "normal", seed=5 * 100003 + 1)     # what adversarial._noise will draw
    noise_g = nn_utils.createNoiseInputs(B, ND, "normal", seed=5 * 100003 + 2)
    pd0, pg0 = host.PARAMETERS_D.copy(), host.PARAMETERS_G.copy()
    c = L.default_context()
    guard0 = c.range_guard_stats()
    adversarial.train(host, real)
    ld, lg = game.batch(real, noise_d, noise_g, want_loss=True)
    assert c.range_guard_stats()[1] == guard0[1], "a host pass ran on bf16x6: the two games did not use one arithmetic"
    pen = host.OPT.D_L2 * float(np.dot(pd0.astype(np.float64), pd0.astype(np.float64))) / 2      # the mirror's f includes the L2 term
    print(f"{method}: loss D device {ld!r} + penalty {pen!r} vs host {host.last_losses['D'][0]!r}; loss G device {lg!r} vs host {host.last_losses['G'][0]!r}")
    assert abs(ld + pen - host.last_losses["D"][0]) <= 1e-5 * max(1.0, abs(ld)), (ld, pen, host.last_losses["D"][0])
    assert np.isfinite(lg)
    game.sync_to_host()
    for which, model, p0, hp, dp in (("D", dev.MODEL_D, pd0, host.PARAMETERS_D, dev.PARAMETERS_D), ("G", dev.MODEL_G, pg0, host.PARAMETERS_G, dev.PARAMETERS_G)):
        d = np.abs(dp.astype(np.float64) - hp)
        print(f"{method} {which}: device game vs host game after one batch: median {np.median(d):.3e}, share above 1e-5 {(d > 1e-5).mean():.3e}, "
              f"max {d.max():.3e} (largest move {np.abs(hp.astype(np.float64) - p0).max():.3e})")
        assert np.all(np.isfinite(dp)) and np.array_equal(dp, _flat(model, lambda n: n.get_params()))
        state = dev.OPTSTATE[method][which]
        cfg = game.hyper_d if which == "D" else game.hyper_g
        for slot, (key, used) in enumerate(zip(L.OPT_STATE_KEYS[method], cfg.slots())):
            if used:
                assert state[key].dtype == np.float32 and np.array_equal(state[key], _flat(model, lambda n: n.optim_state()[slot])), (method, which, key)
        counter = {"adamax": {"t": 1}, "rmsprop": {}}.get(method, {"evalCounter": 1})
        assert {k: state[k] for k in counter} == counter
        assert set(state) == set(host.OPTSTATE[method][which]), (sorted(state), sorted(host.OPTSTATE[method][which]))      # the mirror's own keys
    assert not np.array_equal(dev.PARAMETERS_D, pd0)
    # (rmsprop's first step moves every weight of D by 0.1: D saturates and hands G a gradient of exact zeros - then G rightly stays)
    assert not np.array_equal(dev.PARAMETERS_G, pg0) or not _flat(dev.MODEL_G, lambda n: n.get_grads()).any()
    assert dev.OPTSTATE["adam"] == {"D": {}, "G": {}}
    game.close()
    pd1 = dev.PARAMETERS_D.copy()
    adversarial.train(dev, synth.uniform((B // 2,) + DIMS, 41, 0, 1))                  # the host game continues from the synced state
    assert np.all(np.isfinite(dev.PARAMETERS_D)) and not np.array_equal(dev.PARAMETERS_D, pd1)
    assert dev.OPTSTATE[method]["D"].get("t", dev.OPTSTATE[method]["D"].get("evalCounter", 2)) == 2


def test_device_game_mixed_methods_move_both_nets():
    """D on sgd, G on adam (train.lua:37-38 chooses them independently)"""
    import ganrev._lib as L
    from ganrev import adversarial, synth
    env = _env(D_optmethod="sgd", G_optmethod="adam")
    game = adversarial.DeviceGame(env)
    assert isinstance(game.hyper_d, L.OptimConfig) and isinstance(game.hyper_g, L.Hyper)
    pd0, pg0 = env.PARAMETERS_D.copy(), env.PARAMETERS_G.copy()
    ld, lg = game.batch(synth.uniform((B // 2,) + DIMS, 40, 0, 1), want_loss=True)
    game.sync_to_host()
    assert np.isfinite(ld) and np.isfinite(lg)
    for p, p0 in ((env.PARAMETERS_D, pd0), (env.PARAMETERS_G, pg0)):
        assert np.all(np.isfinite(p)) and not np.array_equal(p, p0)
    assert set(env.OPTSTATE["sgd"]["D"]) == {"learningRate", "momentum", "dfdx", "evalCounter"} and env.OPTSTATE["sgd"]["G"] == {"learningRate": 0.02, "momentum": 0.5}
    assert env.OPTSTATE["adam"] == {"D": {}, "G": {}}
    game.close()
