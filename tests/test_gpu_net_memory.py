"""gpu: who owns the device memory of a net and of a context (csrc/ctx.h DevMem; net.hip ensure_batch, gr_net_create, gr_init / gr_shutdown).
Re-sizing a net's per-batch buffers must change no result and leave no state behind that describes the released buffers; a gr_net_create
that fails must leave its context as it found it; a context that is shut down takes its lazily made buffers with it and disturbs no other.
Nothing here exhausts device memory or asks how much is free: the allocation-failure paths are checked by reading."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS, ND = (1, 32, 32), 16


def _make(kind, seed):
    from ganrev import models, synth
    m = models.create_R(DIMS, ND) if kind == "R" else models.create_G(DIMS, ND)
    synth.init_params(m, seed)
    m.training()
    return m


def _inputs(kind, B):
    from ganrev import synth
    if kind == "R":
        return synth.uniform((B,) + DIMS, 11 + B, 0, 1), synth.normal((B, ND), 21 + B)
    return synth.normal((B, ND), 31 + B), synth.normal((B,) + DIMS, 41 + B)


def _pass(m, kind, B):
    """one training-mode forward + backward at batch B from a fixed seed and forward counter: (output, gradInput, flat gradient)"""
    x, g = _inputs(kind, B)
    out = m.forward(x).copy()          # (the first call compiles the net)
    net = m._net
    net.set_seed(77)                   # restarts the forward counter too: the same Philox noise in every pass
    net.zero_grads()
    out = m.forward(x).copy()
    gin = m.backward(x, g).copy()
    return out, gin, net.get_grads()


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


# The per-batch buffer kinds (net.hip ensure_batch, bwd_conv3) and the stage of these two nets that has each:
#   y, out      every stage (R.7, Linear 512 -> 16, has no pipeline: its out is an alias of y and is not allocated)
#   stat_part   R.0 - R.5 (convolution + BatchNorm), read when the convolution's epilogue wrote the tile sums
#   pool_idx    R.2 and R.5 (SpatialMaxPooling)
#   x_p16       R.1 - R.5 (3x3 convolutions of 64 / 128 input planes); G.3 has one and never uses it (a one-plane output: the few-output kernel)
#   dy pairs    every net: dy_buf / dy_p16 for even stages, dy_buf_b / dy_p16_b for odd ones, g_buf[0..1], in_buf, gout_buf
#   up_tmp      G.1 and G.2 (UpSamplingNearest(2) + convolution): sized by their backward
# x_p16, dy_p16 and the epilogue's stat_part are written only where conv_p16_supported holds, which at batch 2 - 5 of 32 x 32 planes it
# does once "p16_min_tiles" is 1 (as the f16_path fixture sets it): the f16x3 case runs both ways.
@pytest.mark.parametrize("kind", ["R", "G"])
def test_regrowth_keeps_results_and_leaves_no_stale_state(ctx, conv_mode, kind):
    for min_tiles in ((128, 1) if conv_mode == "f16x3" else (128,)):
        ctx.set_tuning("p16_min_tiles", min_tiles)
        try:
            m = _make(kind, 3)
            first = _pass(m, kind, 2)
            grown = _pass(m, kind, 5)          # ensure_batch releases and re-allocates every per-batch buffer
            again = _pass(m, kind, 2)          # fits: nothing moves, and nothing of the B = 5 pass may show
            fresh = _pass(_make(kind, 3), kind, 5)
        finally:
            ctx.set_tuning("p16_min_tiles", 128)       # the library default (conv.hip g_p16_min_tiles)
        assert _same(first, again), (conv_mode, kind, min_tiles)
        assert _same(grown, fresh), (conv_mode, kind, min_tiles)
        assert all(np.isfinite(a).all() for a in first + grown)


def test_failed_creation_leaves_the_context_usable(ctx):
    """Every early return of gr_net_create that a layer list can reach, 50 times each: the code, the message, *out == NULL.  Then a valid net
    in that context computes what it computes in a context that saw no failure.  (The seventh return, "kind %d cannot start a stage", cannot
    be reached: every kind the planner knows is placed in a stage and every other kind is the "unknown kind" case below.)"""
    import ganrev._lib as L
    D = L.LayerDesc
    up = "layer 0: UpSamplingNearest(2) is only fused in front of a 3x3 convolution"
    cases = [   # (layers, input dims, code, message)
        ([D(L.CONV3, 5, 8, 0, 0.0, 0), D(L.ELU, 0, 0, 0, 0.0, 0)], (3, 8, 8), -1, "layer 0: conv expects 5 input planes, got 3"),
        ([D(L.CONV3, 3, 8, 0, 0.0, 0), D(L.BN, 7, 0, 0, 0.0, 0)], (3, 8, 8), -1, "layer 1: BN expects 7 features, got 8"),
        ([D(L.VIEW, 10, 0, 0, 0.0, 0)], (3, 8, 8), -1, "layer 0: view size mismatch"),
        ([D(L.UPSAMPLE2, 0, 0, 0, 0.0, 0)], (3, 8, 8), -2, up),
        ([D(L.UPSAMPLE2, 0, 0, 0, 0.0, 0), D(L.CONVK, 3, 8, 5, 0.0, 0)], (3, 8, 8), -2, up),
        ([D(L.CONV3, 3, 8, 0, 0.0, 0), D(99, 0, 0, 0, 0.0, 0)], (3, 8, 8), -1, "layer 1: unknown kind 99"),
        ([D(L.LINEAR, 10, 4, 0, 0.0, 0)], (3, 8, 8), -1, "layer 0: linear expects 10 inputs, got 192"),
        ([D(L.CONVK, 3, 8, 7, 0.0, 0)], (3, 16, 16), -2, "layer 0: no kernel for a 7x7 convolution (3x3: GR_CONV3; 5x5: GR_CONVK)"),
        ([D(L.CONV3, 3, 8, 0, 0.0, 0), D(L.MAXPOOL2, 0, 0, 0, 0.0, 0)], (3, 1, 1), -1, "layer 1: empty spatial extent"),
    ]
    tried, control = L.Context(ctx.device), L.Context(ctx.device)
    try:
        lib = tried.lib
        for layers, dims, code, msg in cases:
            arr = (D * len(layers))(*layers)
            for _ in range(50):
                net = C.c_void_p(0xdead0)          # (a value the call must overwrite)
                assert lib.gr_net_create(tried.h, arr, len(layers), *dims, C.byref(net)) == code, msg
                assert lib.gr_last_error(tried.h).decode() == msg
                assert net.value is None, msg
        outs = []
        for c in (tried, control):
            m = _make("R", 5)
            m._ctx = c
            outs.append(_pass(m, "R", 2))
            m._net.close()
        assert _same(outs[0], outs[1])
    finally:
        tried.close(); control.close()


def test_a_second_context_opened_and_shut_ten_times(ctx):
    """A context beside the fixture's, ten lives: each makes the buffers a context creates on demand - pin, pin_done and search_state (a
    five-needle search on the small path), head_bar and head_loss_part (two steps of the device-resident trainer, whose head kernel needs them) -
    and gr_shutdown releases them through the context's owner.  The fixture's context computes the same mse before and after."""
    import ganrev._lib as L
    from ganrev import synth
    from ganrev.parallel import DeviceTrainer
    x, t = synth.normal((4, 33), 1), synth.normal((4, 33), 2)
    loss0, grad0 = ctx.mse(x, t)
    N, d = 1 << 17, 32                                  # the smallest table of the small search path (search.hip FILTER_MIN_ROWS)
    emb = np.random.default_rng(3).standard_normal((N, d), dtype=np.float32)
    emb_dev = ctx.upload(emb)
    needles = [5, 77, 4096, 70001, N - 1]
    G, R = _make("G", 1), _make("R", 2)
    idx0 = None
    for life in range(10):
        c2 = L.Context(ctx.device)
        try:
            idx, _ = c2.cosine_topk(None, needles, 3, emb_dev=emb_dev, n=N, d=d)
            assert (idx[:, 0] == needles).all()
            idx0 = idx if idx0 is None else idx0
            assert np.array_equal(idx, idx0)
            for m in (G, R):
                m._ctx, m._net = c2, None               # compile on this context
            G.evaluate(); G.forward(synth.normal((2, ND), 1))
            R.training(); R.forward(synth.uniform((2,) + DIMS, 2, 0, 1)); R.push_params()
            R._net.set_seed(77); R._net.adam_reset()
            tr = DeviceTrainer(c2, G._net, R._net, L.Hyper(), 16)
            losses = []
            for step in range(2):
                tr.new_noise(50 + step); losses.append(tr.step(want_loss=True))
            assert np.isfinite(losses).all()
            tr.close()
            G._net.close(); R._net.close()
        finally:
            c2.close()
    ctx.free(emb_dev)
    loss1, grad1 = ctx.mse(x, t)
    assert loss1 == loss0 and np.array_equal(grad1, grad0)
