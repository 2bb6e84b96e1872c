"""-m gpu: every case of tests/post_paths.py through a one-stage (or conv / Linear + one stage) nn.Sequential: forward and backward once, every
element of every observable (stage output, pool index, running statistics, dy / gradInput, gradWeight, the BatchNorm, bias and slope gradients)
within its float64 bound; then the same pass under set_timing(2): the pipeline labels of the forward and of the backward equal the restated
dispatch, and every result repeats bit for bit.

Element-wise cases run in f32 mode (no convolution: the arithmetic mode does not enter); main-operator cases too - the few-input convolution
that leaves the statistics tiles is fp32 VALU in every mode, and conv_paths' f32 bound then covers the gradient convolutions.  The
operand-ready (g8) kernels need f16x3 and a P16 consumer: producer / consumer pairs with p16_min_tiles = 1, run guarded, lean
(range_guard = 0) and with p16_min_tiles = 128 (test_operand_ready_kernels).  One case sits exactly at the post_big threshold (non-temporal
loads of pass A), its reference computed channel by channel: about 12 s of the module's time on the CPU side.

Cost: the float64 references are numpy passes over at most 1.6 M elements; each GPU call is well under a millisecond."""
import types

import numpy as np
import pytest

import conv_paths as cp
import post_paths as pp

pytestmark = pytest.mark.gpu

ELEM = [c for c in pp.CASES if c.main == "elem"]
MAIN = [c for c in pp.CASES if c.main != "elem" and c.depth == 1]
WORST = {}           # kernel label -> (max |err| / bound, case, observable), printed by the last test
ELU_SEEN = [0.0]     # largest |err| of an ELU output on its negative branch where the input is exact (no BatchNorm in front)


def _counts(ctx):
    out = {}
    for t in ctx.kernel_times():
        out[t["kernel"]] = out.get(t["kernel"], 0) + t["launches"]
    return out


def _delta(after, before):
    return {k: after.get(k, 0) - before.get(k, 0) for k in pp.LABELS if after.get(k, 0) - before.get(k, 0)}


def _note(label, ratio, case, what):
    if ratio > WORST.get(label, (-1.0,))[0]:
        WORST[label] = (ratio, case, what)


def _layer(l, C, linear=False):
    from ganrev import nn
    if l == "bn":
        return nn.BatchNormalization(C) if linear else nn.SpatialBatchNormalization(C)
    if l == "drop":
        return nn.Dropout(pp.P_DROP)
    if l == "sdrop":
        return nn.SpatialDropout(pp.P_SDROP)
    if l == "max":
        return nn.SpatialMaxPooling(2, 2, 2, 2)
    if l == "avg":
        return nn.SpatialAveragePooling(2, 2, 2, 2)
    if l == "LeakyReLU":
        return nn.LeakyReLU(pp.LEAKY_SLOPE)
    return getattr(nn, l)()


def _stage_params(layers, d):
    """the stage's slice of the flat parameter vector, in layer order"""
    out = []
    for l in layers:
        if l == "bn":
            out += [d["gamma"], d["beta"]]
        elif l == "PReLU":
            out.append(np.full(1, d["slope"], np.float32))
    return out


def _set_masks(net, layers, d, first):
    for i, l in enumerate(layers):
        if l in ("drop", "sdrop"):
            behind_pool = any(p in ("max", "avg") for p in layers[:i])
            net.set_mask(first + i, d["keep2" if behind_pool else "keep1"])


def _split_grads(layers, g, C):
    """{observable: values} of the stage's slice g of the flat gradient"""
    out, o = {}, 0
    for l in layers:
        if l == "bn":
            out["ggamma"], out["gbeta"] = g[o:o + C], g[o + C:o + 2 * C]
            o += 2 * C
        elif l == "PReLU":
            out["gslope"] = g[o]
            o += 1
    return out


def _label_of(plan, key, elem):
    if key in ("gin", "gw") and not (elem and key == "gin"):
        return "main operator gradient of the reference dy"
    if key == "out":
        return plan.fwd
    if key in ("run_mean", "run_var"):
        return pp.S_TILES if plan.stats == "tiles" else plan.stats
    if key == "gin":                     # an element-wise stage observes dy as gradInput
        return plan.b or plan.a
    if key == "gbias":
        return pp.BIAS if plan.bias else "post_backward_finalize_kernel"
    if key == "gslope":
        return "prelu_grad_kernel"
    return plan.a         # ggamma, gbeta: pass A's sums (finished by pass B's prologue)


def _compare(case, plan, obs, idx, got):
    ratios = {}
    if idx is not None:
        assert np.array_equal(got["idx"], idx.reshape(-1)), f"{case.name}: pool_index() differs from the reference's argmax in {int((got['idx'] != idx.reshape(-1)).sum())} windows"
    for k, (ref, bound) in obs.items():
        ratios[k] = pp.check(np.asarray(got[k]).reshape(np.shape(ref)), ref, bound, f"{case.name} {k}")
        _note(_label_of(plan, k, case.main == "elem"), ratios[k], case.name, k)
    print(f"{case.name}: max |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + f" [{plan.brief()}]")


def _run_timed(ctx, run):
    got, _ = run(False)
    ctx.set_timing(2)
    try:
        again, labels = run(True)
    finally:
        ctx.set_timing(0)
    return got, again, labels


def _check_labels(case, plan, labels):
    ran_fwd, ran_bwd = labels
    want_bwd = plan.bwd_labels()
    if plan.bias:
        want_bwd[pp.BIAS] = 1
    assert ran_fwd == plan.fwd_labels(), f"{case.name}: the forward launched {ran_fwd}; post_paths predicts {plan.fwd_labels()} - update the mirror if the dispatch changed"
    assert ran_bwd == want_bwd, f"{case.name}: the backward launched {ran_bwd}; post_paths predicts {want_bwd} - update the mirror if the dispatch changed"


@pytest.mark.parametrize("case", ELEM, ids=[c.name for c in ELEM])
def test_elementwise_stage_within_float64_bound(ctx, case):
    import ganrev._lib as L
    from ganrev import nn
    d, _ = pp.inputs(case.name)
    f, plan = case.stage, case.plan()
    obs, idx, r, _ = pp.observables(f, case.training, d)
    if "dy" in obs:
        obs["gin"] = obs.pop("dy")
    y, gout = d["y"], d["gout"]
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f32")
    seq = nn.Sequential()
    for l in case.layers:
        seq.add(_layer(l, case.C))
    (seq.training if case.training else seq.evaluate)()
    try:
        seq.forward(y)                                   # compiles the net
        net = seq._net
        flat = _stage_params(case.layers, d)
        if flat:
            net.set_params(np.concatenate(flat))

        def run(timed):
            if f.bn:
                net.set_bn_running(0, d["rm0"], d["rv0"])
            if case.training:
                _set_masks(net, case.layers, d, 0)
            c0 = _counts(ctx) if timed else None
            got = {"out": net.forward(y)}
            c1 = _counts(ctx) if timed else None
            if f.pool == "max":
                got["idx"] = net.pool_index(case.layers.index("max"), got["out"].size)
            if f.bn and case.training:
                got["run_mean"], got["run_var"] = net.get_bn_running(0)
            if plan.a:
                if net.n_params:
                    net.zero_grads()
                got["gin"] = net.backward(y, gout)
                if net.n_params:
                    got.update(_split_grads(case.layers, net.get_grads(), case.C))
            else:
                with pytest.raises(L.GanrevError, match="requires training mode"):
                    net.backward(y, gout)
            c2 = _counts(ctx) if timed else None
            return got, ((_delta(c1, c0), _delta(c2, c1)) if timed else None)

        got, again, labels = _run_timed(ctx, run)
    finally:
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    _check_labels(case, plan, labels)
    _compare(case, plan, obs, idx, got)
    if case.layers == ("ELU",):          # the input is exact: what is left is the hardware exponential's error
        seen = float(np.abs(got["out"].astype(np.float64) - r["out"])[r["z"] <= 0].max())
        print(f"{case.name}: ELU negative branch on exact inputs, largest |err| {seen:.3e} (bound ELU_ABS + U = {pp.ELU_ABS + pp.U:.3e})")
        assert seen <= pp.ELU_ABS + pp.U
        ELU_SEEN[0] = max(ELU_SEEN[0], seen)
    for k in got:
        assert np.array_equal(got[k], again[k]), f"{case.name} {k}: the timed pass differs from the untimed one"


def _main_inputs(case):
    rng = pp._rng(case.name + " main")
    if case.main == "conv":
        x = rng.standard_normal((case.B, case.cin, case.H, case.W), dtype=np.float32)
        w = (rng.uniform(-1, 1, (case.C, case.cin, 3, 3)) / np.sqrt(case.cin * 9)).astype(np.float32)
    else:
        x = rng.standard_normal((case.B, case.cin), dtype=np.float32)
        w = (rng.uniform(-1, 1, (case.C, case.cin)) / np.sqrt(case.cin)).astype(np.float32)
    return x, w, rng.uniform(-0.5, 0.5, case.C).astype(np.float32)


def _main_grad_refs(case, x, w, dy, Edy, mode="f32"):
    """{gin, gw: (float64 reference, bound)}: the main operator's gradients of the REFERENCE dy - its own arithmetic bound (conv_paths / gemm_paths,
    f32) plus the pipeline's bound on dy carried through |w| and |x|"""
    if case.main == "conv":
        ns = types.SimpleNamespace(mode=mode, up=False, op="net")
        zero, nob = np.zeros(w.shape, np.float32), np.zeros(w.shape[0], np.float32)
        gin, bgin = cp.reference(ns, x, w, nob, dy, zero, op="dgrad")
        gw, bgw = cp.reference(ns, x, w, nob, dy, zero, op="wgrad")
        bgin = bgin + cp.op64("dgrad", cp._t(Edy), cp._t(w).abs(), w.shape).numpy()
        bgw = bgw + cp.op64("wgrad", cp._t(x).abs(), cp._t(Edy), w.shape).numpy()
        return {"gin": (gin, bgin), "gw": (gw, bgw)}
    dy2, E2, x64, w64 = dy.reshape(case.B, case.C), Edy.reshape(case.B, case.C), x.astype(np.float64), w.astype(np.float64)
    gin, gw = dy2 @ w64, dy2.T @ x64
    return {"gin": (gin, pp.U * cp.C_MODE["f32"] * (np.abs(dy2) @ np.abs(w64)) + E2 @ np.abs(w64)),
            "gw": (gw, pp.U * (cp.C_MODE["f32"] * (np.abs(dy2).T @ np.abs(x64)) + np.abs(gw)) + E2.T @ np.abs(x64))}


@pytest.mark.parametrize("case", MAIN, ids=[c.name for c in MAIN])
def test_main_operator_stage_within_float64_bound(ctx, case):
    from ganrev import nn
    x, w, b = _main_inputs(case)
    f, plan = case.stage, case.plan()
    linear = case.main == "linear"
    shape = (case.B, case.C, case.H, case.W)
    d0 = pp.stage_inputs(case.name, f, True, *shape, y=np.zeros(shape, np.float32))        # gamma, beta, running statistics, masks, gradOutput
    gout = d0["gout"].reshape(case.B, case.C) if linear else d0["gout"]
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f32")
    seq = nn.Sequential().add(nn.Linear(case.cin, case.C) if linear else nn.SpatialConvolution(case.cin, case.C, 3, 3, 1, 1, 1, 1))
    for l in case.layers:
        seq.add(_layer(l, case.C, linear))
    seq.training()
    try:
        seq.forward(x)
        net = seq._net
        net.set_params(np.concatenate([w.ravel(), b] + _stage_params(case.layers, d0)))

        def run(timed):
            if f.bn:
                net.set_bn_running(0, d0["rm0"], d0["rv0"])
            _set_masks(net, case.layers, d0, 1)
            c0 = _counts(ctx) if timed else None
            got = {"out": net.forward(x)}
            c1 = _counts(ctx) if timed else None
            got["y"] = net.layer_output(0, shape)
            if f.pool == "max":
                got["idx"] = net.pool_index(1 + case.layers.index("max"), got["out"].size)
            if f.bn:
                got["run_mean"], got["run_var"] = net.get_bn_running(0)
            net.zero_grads()
            got["gin"] = net.backward(x, gout)
            g = net.get_grads()
            got["gw"], got["gbias"] = g[:w.size].reshape(w.shape), g[w.size:w.size + case.C]
            got.update(_split_grads(case.layers, g[w.size + case.C:], case.C))
            c2 = _counts(ctx) if timed else None
            return got, ((_delta(c1, c0), _delta(c2, c1)) if timed else None)

        got, again, labels = _run_timed(ctx, run)
    finally:
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    _check_labels(case, plan, labels)
    d = dict(d0, y=got["y"])
    route = "tiles" if plan.stats == "tiles" else "pass"
    obs, idx, r, bw = pp.observables(f, True, d, route, bias=True)
    kink, pool = pp.violations(f, r)
    assert not kink.any() and (pool is None or not pool.any()), (f"{case.name}: the device's y holds {int(kink.sum())} kink inputs / "
                                                                  f"{0 if pool is None else int(pool.sum())} pool windows inside the margin - choose another seed (case name)")
    dy, Edy = obs.pop("dy")
    obs.update(_main_grad_refs(case, x, w, dy, Edy))
    _compare(case, plan, obs, idx, got)
    for k in got:
        assert np.array_equal(got[k], again[k]), f"{case.name} {k}: the timed pass differs from the untimed one"


def test_chain_of_17_stages_every_bias_gradient(ctx):
    """17 conv(4 -> 4) + BatchNorm stages at 8 x 8: the backward queues 17 bias jobs, the list flushes at 16 - two bias_grad_batch_kernel launches,
    every stage's bias gradient (true value 0: a bias in front of a BatchNorm) within the bound that the reference chain carries down."""
    from ganrev import nn
    case = pp.BY_NAME["chain_17_bias_jobs"]
    f, plan, n = case.stage, case.plan(), case.depth
    shape = (case.B, case.C, case.H, case.W)
    rng = pp._rng(case.name + " main")
    x = rng.standard_normal(shape, dtype=np.float32)
    ws = [(rng.uniform(-1, 1, (case.C, case.C, 3, 3)) / 6.0).astype(np.float32) for _ in range(n)]
    bs = [rng.uniform(-0.5, 0.5, case.C).astype(np.float32) for _ in range(n)]
    ds = [pp.stage_inputs(f"{case.name} {i}", f, True, *shape, y=np.zeros(shape, np.float32)) for i in range(n)]
    gout = ds[-1]["gout"]
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f32")
    seq = nn.Sequential()
    for i in range(n):
        seq.add(nn.SpatialConvolution(case.C, case.C, 3, 3, 1, 1, 1, 1)).add(nn.SpatialBatchNormalization(case.C))
    seq.training()
    try:
        seq.forward(x)
        net = seq._net
        net.set_params(np.concatenate([t for i in range(n) for t in (ws[i].ravel(), bs[i], ds[i]["gamma"], ds[i]["beta"])]))

        def run(timed):
            for i in range(n):
                net.set_bn_running(i, ds[i]["rm0"], ds[i]["rv0"])
            c0 = _counts(ctx) if timed else None
            got = {"out": net.forward(x)}
            c1 = _counts(ctx) if timed else None
            for i in range(n):
                got[f"y{i}"], got[f"out{i}"] = net.layer_output(2 * i, shape), net.layer_output(2 * i + 1, shape)
            net.zero_grads()
            got["gin"] = net.backward(x, gout)
            got["grads"] = net.get_grads()
            c2 = _counts(ctx) if timed else None
            return got, ((_delta(c1, c0), _delta(c2, c1)) if timed else None)

        got, again, (ran_fwd, ran_bwd) = _run_timed(ctx, run)
    finally:
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    want_fwd = {k: n * v for k, v in plan.fwd_labels().items()}
    want_bwd = dict({k: n * v for k, v in plan.bwd_labels().items()}, **{pp.BIAS: pp.bias_launches(n)})
    assert ran_fwd == want_fwd, f"the forward launched {ran_fwd}; post_paths predicts {want_fwd} - update the mirror if the dispatch changed"
    assert ran_bwd == want_bwd, f"the backward launched {ran_bwd}; post_paths predicts {want_bwd} - update the mirror if the dispatch changed"
    per = case.C * case.C * 9 + 3 * case.C
    g, Eg, worst = gout.astype(np.float64), None, {}
    for i in reversed(range(n)):
        d = dict(ds[i], y=got[f"y{i}"])
        r = pp.forward64(f, True, d)
        bw = pp.backward64(f, d, r, gout=g, Eg_in=Eg, bias=True)
        xin = x if i == 0 else got[f"out{i - 1}"]
        refs = _main_grad_refs(case, xin, ws[i], bw["dy"], bw["E_dy"])
        gi = got["grads"][i * per:(i + 1) * per]
        o = ws[i].size
        stage = {"out": (got[f"out{i}"], r["out"], r["E_out"]), "gw": (gi[:o].reshape(ws[i].shape),) + refs["gw"],
                 "gbias": (gi[o:o + case.C], bw["gbias"], bw["E_gbias"]), "ggamma": (gi[o + case.C:o + 2 * case.C], bw["ggamma"], bw["E_ggamma"]),
                 "gbeta": (gi[o + 2 * case.C:], bw["gbeta"], bw["E_gbeta"])}
        if i == 0:
            stage["gin"] = (got["gin"],) + refs["gin"]
        for k, (val, ref, bound) in stage.items():
            worst[k] = max(worst.get(k, 0.0), pp.check(val, ref, bound, f"{case.name} stage {i} {k}"))
        g, Eg = refs["gin"]
    _note(pp.BIAS, worst["gbias"], case.name, "gbias")
    print(f"{case.name}: max |err| / bound over {n} stages " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k in got:
        assert np.array_equal(got[k], again[k]), f"{case.name} {k}: the timed pass differs from the untimed one"


def test_non_temporal_loads_at_post_big(ctx):
    """B 32, C 64, 128 x 128, BatchNorm + ReLU: exactly 128 MB, where launch_post_backward turns the non-temporal loads of pass A on.  The
    reference runs channel by channel (a channel's statistics and decisions are its own)."""
    from ganrev import nn
    case = pp.NT_CASE
    f, plan = case.stage, case.plan()
    assert pp.post_big(case.B, case.C, case.H, case.W) and not pp.post_big(case.B, case.C - 1, case.H, case.W)
    d = pp.stage_inputs(case.name, f, True, case.B, case.C, case.H, case.W)
    chan = lambda c: {k: (v[:, c:c + 1] if k in ("y", "gout") else v[c:c + 1] if isinstance(v, np.ndarray) and v.ndim == 1 else v) for k, v in d.items()}
    for c in range(case.C):
        pp.condition(f, True, chan(c))
    y, gout = d["y"], d["gout"]
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f32")
    seq = nn.Sequential().add(nn.SpatialBatchNormalization(case.C)).add(nn.ReLU())
    seq.training()
    try:
        seq.forward(y[:1])
        net = seq._net
        net.set_params(np.concatenate([d["gamma"], d["beta"]]))

        def run(timed):
            net.set_bn_running(0, d["rm0"], d["rv0"])
            c0 = _counts(ctx) if timed else None
            got = {"out": net.forward(y)}
            c1 = _counts(ctx) if timed else None
            got["run_mean"], got["run_var"] = net.get_bn_running(0)
            net.zero_grads()
            got["gin"] = net.backward(y, gout)
            got.update(_split_grads(case.layers, net.get_grads(), case.C))
            c2 = _counts(ctx) if timed else None
            return got, ((_delta(c1, c0), _delta(c2, c1)) if timed else None)

        got, again, labels = _run_timed(ctx, run)
    finally:
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    _check_labels(case, plan, labels)
    worst = {}
    for c in range(case.C):
        obs, _, r, _ = pp.observables(f, True, chan(c))
        kink, _ = pp.violations(f, r)
        assert not kink.any()
        obs["gin"] = obs.pop("dy")
        for k, (ref, bound) in obs.items():
            val = got[k][:, c:c + 1] if got[k].ndim == 4 else got[k][c:c + 1]
            worst[k] = max(worst.get(k, 0.0), pp.check(val, ref, bound, f"{case.name} channel {c} {k}"))
    for k, v in worst.items():
        _note(_label_of(plan, k, True) + " (non-temporal case)", v, case.name, k)
    print(f"{case.name}: max |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" [{plan.brief()}]")
    for k in got:
        assert np.array_equal(got[k], again[k]), f"{case.name} {k}: the timed pass differs from the untimed one"


@pytest.mark.parametrize("case", pp.G8_CASES, ids=[c.name for c in pp.G8_CASES])
def test_operand_ready_kernels(ctx, case):
    """f16x3 with p16_min_tiles = 1: the producer's pipeline kernel is post_forward_g8_kernel, the consumer's pass B post_backward_b_g8_kernel.
    (1) guarded (the default: the fp32 tensors exist): every element of the g8 output, the pool index, the running statistics and - through the
    reference chain - every gradient within its bound; labels against the mirror; a timed pass repeats the bits.  (2) range_guard = 0 (lean):
    layer_output of the skipped layer is refused, everything else is bit-identical to (1).  (3) p16_min_tiles = 128: the float4 kernel's output
    of the producer stage is bit-identical to the g8 kernel's."""
    import ganrev._lib as L
    from ganrev import nn
    x, w1, b1, w2, b2, d1, d2 = pp.g8_inputs(case)
    f1, f2 = case.stage, pp.Stage(bn=True)
    H2, W2 = case.out_hw
    s1, s2 = (case.B, case.C1, case.H, case.W), (case.B, pp.G8_COUT, H2, W2)
    last1, conv2 = len(case.layers), len(case.layers) + 1
    gout = d2["gout"]
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f16x3")
    seq = nn.Sequential().add(nn.SpatialConvolution(1, case.C1, 3, 3, 1, 1, 1, 1))
    for l in case.layers:
        seq.add(_layer(l, case.C1))
    seq.add(nn.SpatialConvolution(case.C1, pp.G8_COUT, 3, 3, 1, 1, 1, 1)).add(nn.SpatialBatchNormalization(pp.G8_COUT))
    seq.training()
    try:
        ctx.set_tuning("p16_min_tiles", 1)
        seq.forward(x)
        net = seq._net
        net.set_params(np.concatenate([w1.ravel(), b1] + _stage_params(case.layers, d1) + [w2.ravel(), b2, d2["gamma"], d2["beta"]]))

        def run(timed, skipped=False, backward=True):
            net.set_bn_running(0, d1["rm0"], d1["rv0"])
            net.set_bn_running(1, d2["rm0"], d2["rv0"])
            _set_masks(net, case.layers, d1, 1)
            c0 = _counts(ctx) if timed else None
            got = {"out": net.forward(x)}
            c1 = _counts(ctx) if timed else None
            got["y1"], got["y2"] = net.layer_output(0, s1), net.layer_output(conv2, s2)
            if skipped:
                with pytest.raises(L.GanrevError, match="operand-ready"):
                    net.layer_output(last1, (case.B, case.C1, H2, W2))
            else:
                got["out1"] = net.layer_output(last1, (case.B, case.C1, H2, W2))
            if f1.pool == "max":
                got["idx"] = net.pool_index(1 + case.layers.index("max"), case.B * case.C1 * H2 * W2)
            got["rm1"], got["rv1"] = net.get_bn_running(0)
            got["rm2"], got["rv2"] = net.get_bn_running(1)
            if backward:
                net.zero_grads()
                got["gin"] = net.backward(x, gout)
                got["grads"] = net.get_grads()
            c2 = _counts(ctx) if timed else None
            return got, ((_delta(c1, c0), _delta(c2, c1)) if timed else None)

        got, again, (ran_fwd, ran_bwd) = _run_timed(ctx, run)
        p1l, p2l, lean = pp.g8_plans(case, 1, guarded=False)
        ctx.set_tuning("range_guard", 0)
        try:
            lean_got, _ = run(False, skipped=lean)
        finally:
            ctx.set_tuning("range_guard", 1)
        q1, _, _ = pp.g8_plans(case, 128)
        vec_got = None
        if q1.fwd == pp.F_VEC:
            ctx.set_tuning("p16_min_tiles", 128)
            vec_got, _ = run(False, backward=False)
    finally:
        ctx.set_tuning("p16_min_tiles", 128)
        ctx.set_tuning("range_guard", 1)
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    p1, p2, _ = pp.g8_plans(case, 1)
    assert p1.fwd == pp.F_G8, "the case is about the g8 forward kernel"
    add = lambda a, b: {k: a.get(k, 0) + b.get(k, 0) for k in set(a) | set(b)}
    want_fwd, want_bwd = add(p1.fwd_labels(), p2.fwd_labels()), dict(add(p1.bwd_labels(), p2.bwd_labels()), **{pp.BIAS: 1})
    assert ran_fwd == want_fwd, f"{case.name}: the forward launched {ran_fwd}; post_paths predicts {want_fwd} - update the mirror if the dispatch changed"
    assert ran_bwd == want_bwd, f"{case.name}: the backward launched {ran_bwd}; post_paths predicts {want_bwd} - update the mirror if the dispatch changed"
    for k in got:
        assert np.array_equal(got[k], again[k]), f"{case.name} {k}: the timed pass differs from the untimed one"
    # (2) lean against guarded, (3) float4 against g8
    for k in lean_got:
        assert np.array_equal(lean_got[k], got[k]), f"{case.name} {k}: the lean run (range_guard 0) differs from the guarded one"
    if vec_got is not None:
        for k in ("y1", "out1", "rm1", "rv1") + (("idx",) if "idx" in got else ()):
            assert np.array_equal(vec_got[k], got[k]), f"{case.name} {k}: post_forward_vec_kernel (p16_min_tiles 128) differs from post_forward_g8_kernel"
    # (1) the guarded run against float64
    dd1, dd2 = dict(d1, y=got["y1"]), dict(d2, y=got["y2"])
    r1, r2 = pp.forward64(f1, True, dd1, "tiles"), pp.forward64(f2, True, dd2, "tiles")
    kink, pool = pp.violations(f1, r1)
    assert not kink.any() and (pool is None or not pool.any()), f"{case.name}: a decision of the producer stage inside the margin on the device's y - choose another seed"
    ratios = {}

    def chk(key, val, ref, bound, label):
        ratios[key] = pp.check(np.asarray(val).reshape(np.shape(ref)), ref, bound, f"{case.name} {key}")
        _note(label, ratios[key], case.name, key)

    chk("out1", got["out1"], r1["out"], r1["E_out"], pp.F_G8)
    if "idx" in got:
        assert np.array_equal(got["idx"], r1["idx"].reshape(-1)), f"{case.name}: pool_index() differs from the reference's argmax"
    chk("rm1", got["rm1"], r1["run_mean"], r1["E_run_mean"], pp.S_TILES)
    chk("rv1", got["rv1"], r1["run_var"], r1["E_run_var"], pp.S_TILES)
    chk("out", got["out"], r2["out"], r2["E_out"], pp.F_VEC)
    chk("rm2", got["rm2"], r2["run_mean"], r2["E_run_mean"], pp.S_TILES + " (P16 convolution's tiles)")
    chk("rv2", got["rv2"], r2["run_var"], r2["E_run_var"], pp.S_TILES + " (P16 convolution's tiles)")
    bw2 = pp.backward64(f2, dd2, r2, bias=True)
    g = got["grads"]
    n1 = w1.size + case.C1 + sum(t.size for t in _stage_params(case.layers, d1))
    o2 = n1 + w2.size
    lab_b = p2.b + (" (sums)" if p2.b == pp.B_G8 else "")
    chk("gbias2", g[o2:o2 + pp.G8_COUT], bw2["gbias"], bw2["E_gbias"], lab_b)
    chk("ggamma2", g[o2 + pp.G8_COUT:o2 + 2 * pp.G8_COUT], bw2["ggamma"], bw2["E_ggamma"], pp.A_VEC)
    chk("gbeta2", g[o2 + 2 * pp.G8_COUT:o2 + 3 * pp.G8_COUT], bw2["gbeta"], bw2["E_gbeta"], pp.A_VEC)
    if case.full:
        ns = types.SimpleNamespace(main="conv", C=pp.G8_COUT, B=case.B)
        refs2 = _main_grad_refs(ns, got["out1"], w2, bw2["dy"], bw2["E_dy"], "f16x3")
        chk("gw2", g[n1:o2].reshape(w2.shape), *refs2["gw"], "P16 gradient convolutions of the g8 pass B's dy")
        g1, Eg1 = refs2["gin"]
        bw1 = pp.backward64(f1, dd1, r1, gout=g1, Eg_in=Eg1, bias=True)
        o1 = w1.size
        chk("gbias1", g[o1:o1 + case.C1], bw1["gbias"], bw1["E_gbias"], pp.BIAS)
        st = _split_grads(case.layers, g[o1 + case.C1:n1], case.C1)
        chk("ggamma1", st["ggamma"], bw1["ggamma"], bw1["E_ggamma"], "producer behind the P16 data gradient")
        chk("gbeta1", st["gbeta"], bw1["gbeta"], bw1["E_gbeta"], "producer behind the P16 data gradient")
        refs1 = _main_grad_refs(types.SimpleNamespace(main="conv", C=case.C1, B=case.B), x, w1, bw1["dy"], bw1["E_dy"], "f16x3")
        chk("gw1", g[:o1].reshape(w1.shape), *refs1["gw"], "producer behind the P16 data gradient")
        chk("gin", got["gin"], *refs1["gin"], "producer behind the P16 data gradient")
    print(f"{case.name}: max |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + f" [{p1.brief()} | {p2.brief()}]")


def test_report_worst_ratio_per_kernel():
    """(last: prints what the tests above measured, nothing is asserted here - DESIGN.md records these figures.  An observable is credited to a
    label by convention: the stage output to the forward kernel, running statistics to the statistics kernel, dy / an element-wise stage's
    gradInput to pass B (pass A without BatchNorm), the gamma / beta gradients to pass A although pass B's prologue finishes them)"""
    for label in sorted(WORST):
        ratio, case, what = WORST[label]
        print(f"{label}: max |err| / bound {ratio:.3f} ({case} {what})")
    print(f"ELU negative branch on exact inputs: largest |err| {ELU_SEEN[0]:.3e} (asserted in the ELU cases)")
