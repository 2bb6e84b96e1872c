"""-m gpu: every case of tests/generic_paths.py - the pointwise convolution (csrc/conv1x1.hip), the grouped layer kinds (csrc/group.hip) and
the 5x5 weight gradient (csrc/convk.hip) at the shapes where their loops take a second step and their tiles end ragged - as one-stage nets
against float64 with a per-element bound.

Each case: (1) forward, zero_grads, backward: every element of the output, gradInput and every parameter gradient within its bound
(generic_paths.reference: U (c A + |extra|), c measured on the CPU; bias gradients and the multi-slope PReLU by post_paths' rules);
(2) the same pass under set_timing(2): the recorded labels of the three files equal the mirror's, the results repeat bit for bit; (3) a
second backward without zero_grads gives exactly g1 + g1; (4) the 1x1 and grouped kernels are exact fp32 in every GR_CONV_MODE: f32,
bf16x6 and f16x3 give the same bits (the 5x5 case runs in f32 only: its forward takes another kernel in f16x3).

Cost: the references are float64 PyTorch on the CPU, shared through generic_paths' caches (the largest: 520 -> 520 planes over 1225
pixels); each GPU pass is far below a second."""
import numpy as np
import pytest

import ganrev._lib as L
import generic_paths as gp

pytestmark = pytest.mark.gpu


def _pass(net, x, gout):
    out = net.forward(x).copy()
    net.zero_grads()
    gin = net.backward(x, gout).copy()
    return out, gin, net.get_grads()


@pytest.mark.parametrize("case", gp.CASES, ids=[c.name for c in gp.CASES])
def test_generic_path_within_float64_bound(ctx, case):
    d, ref = gp.inputs(case.name), gp.reference(case.name)
    x, gout = d["x"], d["gout"]
    prev = ctx.conv_mode()
    net = L.Net(ctx, case.descs(), case.dims)
    try:
        assert net.n_params == d["params"].size and (net.out_dims[0],) + tuple(net.out_dims[1:]) == (case.Cout, case.H, case.W)
        net.set_params(d["params"])
        ctx.set_conv_mode(case.modes[0])
        got = _pass(net, x, gout)
        ctx.set_timing(2)
        try:
            timed = _pass(net, x, gout)
            names = {t["kernel"] for t in ctx.kernel_times()}
        finally:
            ctx.set_timing(0)
        net.backward(x, gout)
        twice = net.get_grads()
        others = {}
        for mode in case.modes[1:]:
            ctx.set_conv_mode(mode)
            others[mode] = _pass(net, x, gout)
    finally:
        ctx.set_timing(0)
        ctx.set_conv_mode(prev)
        net.close()
    out, gin, grads = got
    nw = case.n_weights
    tensors = {"out": out, "gin": gin}
    tensors.update({"gslope": grads} if case.kind == "pm" else {"gw": grads[:nw], "gb": grads[nw:]})
    assert set(tensors) == set(ref)
    worst = {}
    for k, v in tensors.items():                     # print every figure, then assert
        worst[k] = float(gp.ratio(v, ref[k][0], ref[k][1]).max())
    print(f"{case.name}: max |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in tensors.items():
        gp.check_bound(v, ref[k][0], ref[k][1], f"{case.name} {k}")
    ran = names & gp.UNIVERSE
    assert ran == case.labels(), (f"{case.name}: the net launched {sorted(ran)} (all labels: {sorted(names)}); generic_paths predicts "
                                  f"{sorted(case.labels())} - update the mirror if the launchers changed")
    for what, a, b in zip(("output", "gradInput", "gradients"), got, timed):
        assert np.array_equal(a, b), f"{case.name} {what}: the timed pass differs from the untimed one"
    assert np.array_equal(twice, grads + grads), f"{case.name}: a second backward is not g1 + g1 (max diff {float(np.abs(twice - 2 * grads).max()):.3e})"
    for mode, res in others.items():
        for what, a, b in zip(("output", "gradInput", "gradients"), got, res):
            assert np.array_equal(a, b), f"{case.name} {what}: {mode} differs from {case.modes[0]} (max diff {float(np.abs(a - b).max()):.3e})"
