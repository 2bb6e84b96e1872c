"""-m gpu: every case of tests/p16_paths.py on the operand-ready (P16) convolution kernels, f16x3 with p16_min_tiles = 1.

Training pairs (producer conv(1 -> C1) + BatchNorm + activation [+ average pool] [+ dropout], consumer conv(C1 -> C2) + BatchNorm).  The guarded
run (range_guard = 1: the fp32 copies exist) is held to float64: the consumer's RAW output y2 element by element against conv64(out1, w2) + b2,
out1 being the producer output the image was split from - the check no other module makes - then the running statistics, the net output and,
through the reference chain, every gradient (backward64 with Eg_in; the convolutions' arithmetic bound with the P16 operands' scale magnitudes
plus the pipeline's bound on dy carried through |w| and |x|).  Then the lean rerun (range_guard = 0) and the rerun under the per-kernel timer
must repeat every still-observable result bit for bit, and the timed pass's P16 labels, forward and backward apart, must equal the mirror.

evaluate() chains: the net output (and the raw output of a pooling stage) against the bound propagated along the float64 chain, with
eval_p16 = 1 and, as the control that the bound is not tailored to the hand-over, with eval_p16 = 0; the convolution labels of both runs.

Cost: the float64 references (torch convolutions, numpy pipeline) dominate; the largest are the 63-image, 1024-channel cases."""
import numpy as np
import pytest

import conv_paths as cp
import p16_paths as p16
import post_paths as pp
from test_gpu_post_paths import _layer, _set_masks, _split_grads, _stage_params

pytestmark = pytest.mark.gpu

WORST = {}           # kernel label -> (max |err| / bound, case, observable), printed by the last test
SEEN = set()         # every P16 label an asserted label set held
RAN = set()          # the cases that ran (the last test asserts SEEN only behind a whole run)


def _note(label, ratio, case, what):
    if ratio > WORST.get(label, (-1.0,))[0]:
        WORST[label] = (ratio, case, what)


def _counts(ctx):
    out = {}
    for t in ctx.kernel_times():
        out[t["kernel"]] = out.get(t["kernel"], 0) + t["launches"]
    return out


def _delta(after, before, keep):
    return {k: after[k] - before.get(k, 0) for k in after if keep(k) and after[k] - before.get(k, 0)}


def check_training(case, inp, got):
    """The guarded run of a training pair against float64 -> {observable: max |err| / bound}"""
    x, w1, b1, w2, b2, d1, d2 = inp
    f1, f2 = case.stage, pp.Stage(bn=True)
    r = p16.train_route(case)
    ratios = {}

    def chk(key, val, ref, bound, label, conv=False):
        check = cp.check_bound if conv else pp.check
        ratios[key] = check(np.asarray(val).reshape(np.shape(ref)), ref, bound, f"{case.name} {key}")
        _note(label, ratios[key], case.name, key)

    dd1 = dict(d1, y=got["y1"])
    r1 = pp.forward64(f1, True, dd1, "tiles")
    chk("out1", got["out1"], r1["out"], r1["E_out"], pp.F_G8)
    chk("rm1", got["rm1"], r1["run_mean"], r1["E_run_mean"], pp.S_TILES)
    chk("rv1", got["rv1"], r1["run_var"], r1["E_run_var"], pp.S_TILES)
    # the image's scale magnitude: restated from the device's y1, an upper estimate of the slot - and of the tensor
    Bd = p16.bound_fwd(f1, got["y1"], d1["gamma"], d1["beta"])
    assert float(np.abs(got["out1"]).max()) <= Bd, f"{case.name}: the a-priori bound {Bd} lies below max|out1|"
    # THE check of this module: the consumer's raw output against a float64 convolution of exactly what its input image was split from
    y2, By2 = p16.conv_ref("fwd", got["out1"], w2, b2, None, a_scale=Bd)
    chk("y2", got["y2"], y2, By2, case.fwd, conv=True)
    dd2 = dict(d2, y=got["y2"])
    r2 = pp.forward64(f2, True, dd2, "tiles")
    tiles2 = pp.S_TILES + " (P16 convolution's tiles)"
    chk("out", got["out"], r2["out"], r2["E_out"], pp.F_VEC)
    chk("rm2", got["rm2"], r2["run_mean"], r2["E_run_mean"], tiles2)
    chk("rv2", got["rv2"], r2["run_var"], r2["E_run_var"], tiles2)
    if not case.backward:
        return ratios
    bw2 = pp.backward64(f2, dd2, r2, bias=True)
    Bdy = p16.bound_dy(got["y2"], d2["gamma"], float(np.abs(bw2["dz"]).max()))
    assert float(np.abs(bw2["dy"]).max()) <= Bdy
    g = got["grads"]
    n1 = w1.size + case.C1 + sum(t.size for t in _stage_params(case.layers, d1))
    o2 = n1 + w2.size
    chk("gbias2", g[o2:o2 + case.C2], bw2["gbias"], bw2["E_gbias"], r.p2.b + (" (sums)" if r.p2.b == pp.B_G8 else ""))
    chk("ggamma2", g[o2 + case.C2:o2 + 2 * case.C2], bw2["ggamma"], bw2["E_ggamma"], pp.A_VEC)
    chk("gbeta2", g[o2 + 2 * case.C2:o2 + 3 * case.C2], bw2["gbeta"], bw2["E_gbeta"], pp.A_VEC)
    wg, dg = r.wgrad is not None, r.dgrad is not None
    gw2, Bgw2 = p16.conv_ref("wgrad", got["out1"], w2, None, bw2["dy"], a_scale=Bd if wg else None, b_scale=Bdy if wg else None, E_b=bw2["E_dy"])
    chk("gw2", g[n1:o2].reshape(w2.shape), gw2, Bgw2, r.wgrad["label"] + " + reduce_tiled" if wg else "split weight gradient behind a P16 forward", conv=True)
    g1, Eg1 = p16.conv_ref("dgrad", None, w2, None, bw2["dy"], a_scale=Bdy if dg else None, E_a=bw2["E_dy"])
    behind = (r.dgrad[0] + " as data gradient") if dg else "split data gradient behind a P16 forward"
    bw1 = pp.backward64(f1, dd1, r1, gout=g1, Eg_in=Eg1, bias=True)
    o1 = w1.size
    chk("gbias1", g[o1:o1 + case.C1], bw1["gbias"], bw1["E_gbias"], behind)
    st = _split_grads(case.layers, g[o1 + case.C1:n1], case.C1)
    chk("ggamma1", st["ggamma"], bw1["ggamma"], bw1["E_ggamma"], behind)
    chk("gbeta1", st["gbeta"], bw1["gbeta"], bw1["E_gbeta"], behind)
    gw1, Bgw1 = p16.conv_ref("wgrad", x, w1, None, bw1["dy"], E_b=bw1["E_dy"])
    chk("gw1", g[:o1].reshape(w1.shape), gw1, Bgw1, behind, conv=True)
    gin, Bgin = p16.conv_ref("dgrad", None, w1, None, bw1["dy"], E_a=bw1["E_dy"])
    chk("gin", got["gin"], gin, Bgin, behind, conv=True)
    return ratios


@pytest.mark.parametrize("case", p16.TRAIN_CASES, ids=[c.name for c in p16.TRAIN_CASES])
def test_training_pair_within_float64_bound(ctx, case):
    import ganrev._lib as L
    from ganrev import nn
    inp = p16.train_inputs(case)
    x, w1, b1, w2, b2, d1, d2 = inp
    H2, W2 = case.out_hw
    s1, s2, so1 = (case.B, case.C1, case.H, case.W), (case.B, case.C2, H2, W2), (case.B, case.C1, H2, W2)
    last1, conv2 = len(case.layers), len(case.layers) + 1
    gout = d2["gout"]
    lean = p16.train_route(case, guarded=False).lean
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f16x3")
    seq = nn.Sequential().add(nn.SpatialConvolution(1, case.C1, 3, 3, 1, 1, 1, 1))
    for l in case.layers:
        seq.add(_layer(l, case.C1))
    seq.add(nn.SpatialConvolution(case.C1, case.C2, 3, 3, 1, 1, 1, 1)).add(nn.SpatialBatchNormalization(case.C2))
    seq.training()
    try:
        ctx.set_tuning("p16_min_tiles", 1)
        seq.forward(x)
        net = seq._net
        net.set_params(np.concatenate([w1.ravel(), b1] + _stage_params(case.layers, d1) + [w2.ravel(), b2, d2["gamma"], d2["beta"]]))

        def run(timed, skipped=False):
            net.set_bn_running(0, d1["rm0"], d1["rv0"])
            net.set_bn_running(1, d2["rm0"], d2["rv0"])
            _set_masks(net, case.layers, d1, 1)
            c0 = _counts(ctx) if timed else None
            got = {"out": net.forward(x)}
            c1 = _counts(ctx) if timed else None
            got["y1"], got["y2"] = net.layer_output(0, s1), net.layer_output(conv2, s2)
            if skipped:
                with pytest.raises(L.GanrevError, match="operand-ready"):
                    net.layer_output(last1, so1)
            else:
                got["out1"] = net.layer_output(last1, so1)
            got["rm1"], got["rv1"] = net.get_bn_running(0)
            got["rm2"], got["rv2"] = net.get_bn_running(1)
            if case.backward:
                net.zero_grads()
                got["gin"] = net.backward(x, gout)
                got["grads"] = net.get_grads()
            c2 = _counts(ctx) if timed else None
            keep = lambda k: k in p16.P16_LEAVES
            return got, ((_delta(c1, c0, keep), _delta(c2, c1, keep)) if timed else None)

        got, _ = run(False)
        ctx.set_timing(2)
        try:
            timed_got, (ran_fwd, ran_bwd) = run(True)
        finally:
            ctx.set_timing(0)
        ctx.set_tuning("range_guard", 0)
        lean_got, _ = run(False, skipped=lean)
    finally:
        ctx.set_tuning("p16_min_tiles", 128)       # the library defaults (conv.hip g_p16_min_tiles, ctx.h range_guard)
        ctx.set_tuning("range_guard", 1)
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    want_fwd, want_bwd = case.mirror()
    assert ran_fwd == want_fwd, f"{case.name}: the forward launched {ran_fwd}; p16_paths predicts {want_fwd} - update the mirror if the dispatch changed"
    assert ran_bwd == want_bwd, f"{case.name}: the backward launched {ran_bwd}; p16_paths predicts {want_bwd} - update the mirror if the dispatch changed"
    SEEN.update(ran_fwd, ran_bwd)
    RAN.add(case.name)
    for k in got:
        assert np.array_equal(got[k], timed_got[k]), f"{case.name} {k}: the timed pass differs from the untimed one"
    assert set(lean_got) == set(got) - ({"out1"} if lean else set())
    for k in lean_got:
        assert np.array_equal(lean_got[k], got[k]), f"{case.name} {k}: the lean run (range_guard 0) differs from the guarded one"
    ratios = check_training(case, inp, got)
    print(f"{case.name}: max |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def check_evaluate(case, chain, out, raw, labels, eval_p16):
    """one evaluate() run against the propagated bound -> {observable: max |err| / bound}; labels: the convolution kernels in launch order"""
    ref, E, _, raws = chain
    ratios = {"out": pp.check(out, ref, E, f"{case.name} eval_p16 = {eval_p16} out")}
    for i, y in raw.items():
        ratios[f"y{i}"] = pp.check(y, raws[i][0], raws[i][1], f"{case.name} eval_p16 = {eval_p16} stage {i} raw output")
    if eval_p16:
        for k in labels:
            _note(k + " (evaluate() chain)", ratios["out"], case.name, "out")
    return ratios


@pytest.mark.parametrize("case", p16.EVAL_CASES, ids=[c.name for c in p16.EVAL_CASES])
def test_evaluate_chain_within_propagated_bound(ctx, case):
    from ganrev import nn
    x, params = p16.eval_inputs(case.name)
    chain = p16.eval_chain(case, x, params)
    st = case.stages()
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f16x3")
    seq, main, flat = nn.Sequential(), {}, []
    for i, ((cin, co, h, w, act, pool), (wt, b, gamma, beta, rm, rv)) in enumerate(zip(st, params)):
        main[i] = len(seq.modules)
        seq.add(nn.SpatialConvolution(cin, co, 3, 3, 1, 1, 1, 1)).add(nn.SpatialBatchNormalization(co)).add(_layer(act, co))
        if pool:
            seq.add(_layer("avg", co))
        flat += [wt.ravel(), b, gamma, beta]
    seq.evaluate()
    conv = lambda k: k.startswith("conv3x3_")
    runs = {}
    try:
        ctx.set_tuning("p16_min_tiles", 1)
        seq.forward(x)
        net = seq._net
        net.set_params(np.concatenate(flat))
        for i, p in enumerate(params):
            net.set_bn_running(i, p[4], p[5])
        for v in (1, 0):
            ctx.set_tuning("eval_p16", v)
            out = net.forward(x).copy()
            raw = {i: net.layer_output(main[i], (case.B, s[1], s[2], s[3])) for i, s in enumerate(st) if s[5]}
            ctx.set_timing(2)
            try:
                c0 = _counts(ctx)
                again = net.forward(x).copy()
                ran = _delta(_counts(ctx), c0, conv)
            finally:
                ctx.set_timing(0)
            runs[v] = (out, raw, again, ran)
    finally:
        ctx.set_tuning("eval_p16", 1)              # the library defaults (net.hip g_eval_p16, conv.hip g_p16_min_tiles)
        ctx.set_tuning("p16_min_tiles", 128)
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    for v, want in ((1, case.on), (0, case.off)):
        out, raw, again, ran = runs[v]
        counts = {k: want.count(k) for k in want}
        assert ran == counts, f"{case.name} eval_p16 = {v}: the forward launched {ran}; p16_paths predicts {counts} - update the mirror if the dispatch changed"
        assert np.array_equal(out, again), f"{case.name} eval_p16 = {v}: the timed pass differs from the untimed one"
        ratios = check_evaluate(case, chain, out, raw, want, v)
        print(f"{case.name} eval_p16 = {v}: max |err| / bound " + ", ".join(f"{k} {r:.4f}" for k, r in ratios.items()))
    assert not any("_po_" in k or "p16o" in k for k in runs[0][3])
    # (a power-of-two scale commutes with the fp16 split unless a low term leaves the normal range: the two runs differ in few elements or none)
    print(f"{case.name}: {int((runs[1][0] != runs[0][0]).sum())} of {runs[1][0].size} output elements differ between eval_p16 = 1 and 0")
    SEEN.update(k for k in runs[1][3] if k in p16.P16_LEAVES)
    RAN.add(case.name)


def test_report_worst_ratio_per_kernel():
    """(last: every P16 label was in an asserted label set of the tests above; prints what they measured - DESIGN.md records these figures.  y2 is
    credited to the consumer's forward kernel, gw2 to the weight-gradient pair, the producer's gradients to the data-gradient kernel in front
    of them; an evaluate() chain's output to every kernel of the chain)"""
    if RAN == {c.name for c in p16.TRAIN_CASES + p16.EVAL_CASES}:         # (a run of a selection has less to report)
        assert SEEN == p16.P16_LEAVES, f"P16 labels no asserted label set held: {sorted(p16.P16_LEAVES - SEEN)}"
    for label in sorted(WORST):
        ratio, case, what = WORST[label]
        print(f"{label}: max |err| / bound {ratio:.4f} ({case} {what})")
