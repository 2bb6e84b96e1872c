"""-m gpu: every case of tests/gemm_paths.py through a one-stage nn.Sequential holding one nn.Linear, against float64 with a per-element
bound, and the GEMM labels each pass records under the per-kernel timer against the restated dispatch.

csrc/gemm.hip holds three MFMA kernels in four operand-stride instantiations each and a split-K reduce; launch_gemm picks among them by
mode, shape and plan, and the kernels fork again on vector / scalar loads, the two store paths, accumulate, the place of the bias and the
fused evaluate()-mode epilogue.  Each case: (1) forward, set_grads(g0), backward: every element of the output, gradInput and gradWeight
within U * (c A + [f16x3 kernel] C16 M) + U |bias or accumulated result| of the float64 result (gemm_paths.reference), gradBias within
U * (8 colsum|dy| + |result|); (2) the same pass under set_timing(2): the GEMM label of the forward, and the two of the backward, equal
gemm_paths' prediction, the reduce kernel ran exactly once per split plan, and every result repeats bit for bit (split-K is ordered and
uses no atomics).  Epilogue cases run the forward only, in evaluate() mode: the stand-alone pipeline kernel is absent exactly when the
mirror says fused, and the output lies within the bound propagated through BatchNorm + activation (gemm_paths.reference_epilogue).

Cost: float64 references are numpy matrix products of at most 257 x 2052 x 640; each GPU pass is well under a millisecond."""
import numpy as np
import pytest

import gemm_paths as gp

pytestmark = pytest.mark.gpu


def _counts(ctx):
    """label -> launches so far under the timer (the table is cumulative since set_timing(2))"""
    out = {}
    for t in ctx.kernel_times():
        out[t["kernel"]] = out.get(t["kernel"], 0) + t["launches"]
    return out


def _delta(after, before, labels):
    return {k: after.get(k, 0) - before.get(k, 0) for k in labels if after.get(k, 0) - before.get(k, 0)}


def _expected(launches):
    """label -> launches of the given Launch records"""
    out = {}
    for l in launches:
        out[l.kernel] = out.get(l.kernel, 0) + 1
        if l.reduces:
            out[gp.REDUCE] = out.get(gp.REDUCE, 0) + l.reduces
    return out


def _sequential(case):
    from ganrev import nn
    seq = nn.Sequential().add(nn.Linear(case.nin, case.nout))
    if case.bn:
        seq.add(nn.BatchNormalization(case.nout))
    if case.act != "none":
        seq.add(nn.LeakyReLU(gp.LEAKY_SLOPE) if case.act == "LeakyReLU" else getattr(nn, case.act)())
    return seq


@pytest.mark.parametrize("case", gp.CASES, ids=[c.name for c in gp.CASES])
def test_gemm_path_within_float64_bound(ctx, case):
    from ganrev import synth
    d = gp.inputs(case)
    x, w, b, dy = d["x"], d["w"], d["b"], d["dy"]
    mirror = case.launches()
    if case.post:
        refs = {"fwd": gp.reference_epilogue(case, d)}
    else:
        refs = {op: gp.reference(case, op, d) for op in gp.OPS}
        refs["gbias"] = gp.reference_grad_bias(d)
    prev = ctx.conv_mode()
    ctx.set_conv_mode(case.mode)
    seq = _sequential(case)
    synth.init_params(seq, 1)
    if case.post:
        seq.evaluate()
    try:
        seq.forward(x)                                  # compiles the net, in the Sequential's mode
        net = seq._net
        mean, var, gamma, beta = d["bn"]
        net.set_params(np.concatenate([w.ravel(), b] + ([gamma, beta] if case.bn else [])))
        if case.bn:
            net.set_bn_running(0, mean, var)
        g0 = np.concatenate([d["gw0"].ravel(), d["gb0"]])

        def run(timed):
            """-> results by operation, and (timed) the labels of the forward and of the backward"""
            c0 = _counts(ctx) if timed else None
            out = {"fwd": net.forward(x)}
            c1 = _counts(ctx) if timed else None
            if not case.post:
                net.set_grads(g0)
                out["dgrad"] = net.backward(x, dy)
                g = net.get_grads()
                out["wgrad"], out["gbias"] = g[:w.size].reshape(w.shape), g[w.size:]
            c2 = _counts(ctx) if timed else None
            labels = gp.LABELS | gp.POST_LABELS
            return out, (_delta(c1, c0, labels), _delta(c2, c1, labels)) if timed else None

        got, _ = run(False)
        ctx.set_timing(2)
        try:
            again, (ran_fwd, ran_bwd) = run(True)
        finally:
            ctx.set_timing(0)
    finally:
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    # the labels first: a dispatch that moved is reported as that, not as the numeric failure it may cause
    want_fwd = _expected([mirror["fwd"]])
    if mirror["fwd"].epilogue == "refused":
        want_fwd[gp.POST_FORWARD] = 1                   # the stand-alone pipeline kernel; absent when the epilogue is fused
    assert ran_fwd == want_fwd, f"{case.name}: the forward launched {ran_fwd}; gemm_paths predicts {want_fwd} - update the mirror if the dispatch changed"
    if not case.post:
        want_bwd = _expected([mirror["wgrad"], mirror["dgrad"]])
        assert ran_bwd == want_bwd, f"{case.name}: the backward launched {ran_bwd}; gemm_paths predicts {want_bwd} - update the mirror if the dispatch changed"
    worst = {op: gp.check_bound(got[op], *refs[op], f"{case.name} {op}") for op in refs}
    print(f"{case.name}: max |err| / bound " + ", ".join(f"{op} {worst[op]:.3f} [{mirror[op].brief() if op in mirror else 'bias job'}]" for op in refs))
    for op in got:
        assert np.array_equal(got[op], again[op]), f"{case.name} {op}: the timed pass differs from the untimed one"
