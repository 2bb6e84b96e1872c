"""-m gpu: every case of tests/conv_paths.py through the stand-alone convolution entry points, against float64 with a per-element bound,
and the kernel labels each call records under the per-kernel timer against the restated dispatch.

gr_conv3_forward_dev / gr_conv3_backward_data_dev / gr_conv3_backward_weight_dev pick among 55 kernel instantiations by mode, shape and the
stack8_min_wgs knob; one-stage nets reach the 12 that only a net launches (few-input, 5x5).  Each case: (1) one call, every element within u * (c_mode * A + [f16x3] C16 * M) + u * |bias or accumulated result| of
the float64 result (conv_paths.reference: the constants and their derivation are there); (2) the same call under set_timing(2): the
convolution labels it records equal what conv_paths predicts, and the result is bit-identical to the untimed call.

Cost: references are float64 torch on the CPU (a few large cases, the persistent-grid ones, dominate); each GPU call is well under a
millisecond."""
import numpy as np
import pytest

import conv_paths as cp

pytestmark = pytest.mark.gpu


def _run(ctx, case, dev):
    """One call of the case's entry point on device buffers dev = (x, w, b, dy, out); returns the result as float32 numpy."""
    lib, c = ctx.lib, case
    dx, dw, db, ddy, dout = dev
    if c.op == "fwd":
        ctx.check(lib.gr_conv3_forward_dev(ctx.h, dx, dw, db, dout, c.B, c.Cin, c.Cout, c.H, c.W, 1 if c.up else 0), "fwd")
        return ctx.download(dout, (c.B, c.Cout, c.H, c.W))
    if c.op == "dgrad":
        ctx.check(lib.gr_conv3_backward_data_dev(ctx.h, ddy, dw, dout, c.B, c.Cin, c.Cout, c.H, c.W), "bwd-data")
        return ctx.download(dout, (c.B, c.Cin, c.H, c.W))
    ctx.check(lib.gr_conv3_backward_weight_dev(ctx.h, dx, ddy, dout, c.B, c.Cin, c.Cout, c.H, c.W), "bwd-weight")
    ctx.synchronize()
    return ctx.download(dout, (c.Cout, c.Cin, 3, 3))


@pytest.mark.parametrize("case", cp.CASES, ids=[c.name for c in cp.CASES])
def test_conv_path_within_float64_bound(ctx, case):
    x, w, b, dy, gw0 = cp.inputs(case)
    ref, bound = cp.reference(case, x, w, b, dy, gw0)
    out_shape = {"fwd": (case.B, case.Cout, case.H, case.W), "dgrad": x.shape, "wgrad": gw0.shape}[case.op]
    up = lambda a: ctx.upload(np.ascontiguousarray(a, np.float32))
    dev = [up(x), up(w), up(b), up(dy), up(gw0) if case.op == "wgrad" else ctx.malloc(4 * int(np.prod(out_shape)))]
    prev = ctx.conv_mode()
    ctx.set_conv_mode(case.mode)
    ctx.set_tuning("stack8_min_wgs", case.stack8)
    try:
        got = _run(ctx, case, dev)
        if case.op == "wgrad":
            ctx.upload(gw0, dev[4])                     # the weight gradient accumulates: the timed call starts from gw0 again
        ctx.set_timing(2)
        try:
            again = _run(ctx, case, dev)
            names = {t["kernel"] for t in ctx.kernel_times()}
        finally:
            ctx.set_timing(0)
    finally:
        ctx.set_tuning("stack8_min_wgs", 128)           # the library default (conv.hip g_stack8_min_wgs)
        ctx.set_conv_mode(prev)
        for p in dev:
            ctx.free(p)
    worst = cp.check_bound(got, ref, bound, case.name)
    print(f"{case.name}: max |err| / bound {worst:.3f}")
    ran = names & cp.LEAVES
    assert ran == case.leaves(), (f"{case.name}: the library launched {sorted(ran)} (all labels: {sorted(names)}); conv_paths predicts "
                                  f"{sorted(case.leaves())} - update the mirror if the dispatch changed")
    assert np.array_equal(again, got), f"{case.name}: the timed call differs from the untimed one"


@pytest.mark.parametrize("case", cp.NET_CASES, ids=[c.name for c in cp.NET_CASES])
def test_net_conv_path_within_float64_bound(ctx, case):
    """The kernels only a net launches (few input channels; 5x5 split and fp32 direct kernels): a one-stage net whose input is the net
    input and whose output is the raw convolution.  Forward, gradInput and the weight gradient (gr_net_get_grads) against the same bound;
    the net-only kernels forward + backward record under the timer equal conv_paths.net_stage_leaves, and the timed pass repeats the bits."""
    from ganrev import nn, synth
    x, w, b, dy, gw0 = cp.inputs(case)
    refs = {op: cp.reference(case, x, w, b, dy, gw0, op) for op in ("fwd", "dgrad", "wgrad")}
    prev = ctx.conv_mode()
    ctx.set_conv_mode(case.mode)
    k, pad = case.ksz, case.ksz // 2
    seq = nn.Sequential().add(nn.SpatialConvolution(case.Cin, case.Cout, k, k, 1, 1, pad, pad))
    synth.init_params(seq, 1)
    try:
        seq.forward(x)                                  # compiles the net
        net = seq._net
        net.set_params(np.concatenate([w.ravel(), b.ravel()]))

        def run():
            y = net.forward(x)
            net.zero_grads()
            gin = net.backward(x, dy)
            return y, gin, net.get_grads()[:w.size].reshape(w.shape)

        got = run()
        ctx.set_timing(2)
        try:
            again = run()
            names = {t["kernel"] for t in ctx.kernel_times()}
        finally:
            ctx.set_timing(0)
    finally:
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    worst = [cp.check_bound(g, *refs[op], f"{case.name} {op}") for g, op in zip(got, ("fwd", "dgrad", "wgrad"))]
    print(f"{case.name}: max |err| / bound fwd {worst[0]:.3f}, gradInput {worst[1]:.3f}, gradWeight {worst[2]:.3f}")
    ran = names & cp.NET_LEAVES
    assert ran == case.leaves(), (f"{case.name}: the net launched {sorted(ran)} (all labels: {sorted(names)}); conv_paths predicts "
                                  f"{sorted(case.leaves())} - update the mirror if the dispatch changed")
    for g, a, op in zip(got, again, ("fwd", "dgrad", "wgrad")):
        assert np.array_equal(g, a), f"{case.name} {op}: the timed pass differs from the untimed one"
