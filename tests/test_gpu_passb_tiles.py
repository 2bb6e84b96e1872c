"""-m gpu: the tile loop of post_backward_b_g8_kernel (a compile-time count of float4 groups per thread and tile, the SpatialDropout word fetched
once per image) and the two bodies of post_backward_a_vec_kernel (single round / several rounds with a second buffer set), at the smallest
shapes at which they can go wrong.  The machinery is tests/post_paths.py's and tests/test_gpu_post_paths.py's, imported as it is.

f16x3, p16_min_tiles = 1.  Two placements of the stage under test:
  producer   conv(1 -> 64) + BatchNorm + stage, then conv(64 -> 64) + BatchNorm: post_paths.G8Case through test_operand_ready_kernels itself.  The
             operand-ready pass B is the CONSUMER's, a bare BatchNorm: the generic instantiation (combo 0) of the kernel.
  consumer   conv(1 -> 64) + BatchNorm + ELU + Dropout, then conv(64 -> 64) + BatchNorm + stage: the operand-ready pass B runs the stage itself, i.e.
             the instantiations of combos 1, 2 (max pool + Dropout) and 3 (SpatialDropout + max pool) that R's training step launches.
Shapes: 16 x 16 planes (one 256-pixel tile per plane: the block's next tile is the next image's), 32 x 32 (four tiles per plane); B = 1 (one
block per group, nothing behind its image), 3, 257 (129 batch slices: two images in all but the last, which holds one).  Every case runs guarded
(the fp32 dy is kept) and lean (range_guard = 0: dy exists operand-ready only).

Assertions, as test_operand_ready_kernels: every gradient within the float64 bound of post_paths / conv_paths, the labels against the restated
dispatch, a second (timed) run repeats every bit, the lean run repeats every bit.  B = 257: the convolution gradients are compared between the
runs only (full = False there too: the cost of the float64 convolutions); a max pool needs a seed whose windows hold no near-tie on the device's y
(post_paths CONDITIONING) - found on the CPU for B = 1 and B = 3, out of reach for the 10^6 windows of B = 257, which therefore runs combo 1.

Pass A: element-wise stages whose block owns exactly one round of 1024 float4 groups (the single-round body) and the B = 29 case of one round and
a half (the body with the second buffer set); the launcher's rule is restated here and asserted on the geometry."""
import dataclasses
import types

import numpy as np
import pytest

import conv_paths as cp
import post_paths as pp
import test_gpu_post_paths as tg

pytestmark = pytest.mark.gpu

CB = {1: ("bn", "ELU", "drop"), 2: ("bn", "ELU", "max", "drop"), 3: ("bn", "ELU", "sdrop", "max")}

# ---------------------------------------------------------------- producer placement: G8Case, run by test_operand_ready_kernels
_G8 = "F:g8 S:tiles A:vec/1 B:vec/1 bias"
_C64 = "cb0 F:vec S:tiles A:vec/1 B:g8/"
PRODUCER = [
    pp.G8Case("p_32x32_b3_cb1", 3, 64, 32, 32, CB[1], ("cb1 " + _G8, _C64 + "3 bias", "lean")),                    # four tiles per plane, three blocks per group
    pp.G8Case("p_16x16_b1_cb1", 1, 64, 16, 16, CB[1], ("cb1 " + _G8, _C64 + "1 bias", "lean")),                    # one tile, one image
    pp.G8Case("p_max_from_32_b1_cb3", 1, 64, 32, 32, CB[3], ("cb3 " + _G8, _C64 + "1 bias", "lean"), seed=4),      # the consumer's planes are 16 x 16
]


@pytest.mark.parametrize("case", PRODUCER, ids=[c.name for c in PRODUCER])
def test_passb_generic_behind_a_producer_stage(ctx, case):
    p1, p2, lean = pp.g8_plans(case, 1, guarded=False)
    assert (p1.brief(), p2.brief(), "lean" if lean else "kept") == case.expect
    assert p2.b == pp.B_G8
    tg.test_operand_ready_kernels(ctx, case)


# ---------------------------------------------------------------- consumer placement
@dataclasses.dataclass(frozen=True)
class ConsumerCase:
    name: str
    B: int
    H: int
    W: int
    combo: int
    slices: int              # grid.y of the operand-ready pass B, by hand: min(B, 256) re-derived from `per`
    seed: int = 0
    full: bool = True

    @property
    def stage(self):
        return pp.stage_of(CB[self.combo], True)


CONSUMER = [
    ConsumerCase("c_16x16_b1_cb1", 1, 16, 16, 1, 1),
    ConsumerCase("c_16x16_b3_cb1", 3, 16, 16, 1, 3),
    ConsumerCase("c_32x32_b3_cb1", 3, 32, 32, 1, 3),
    ConsumerCase("c_32x32_b1_cb1", 1, 32, 32, 1, 1),
    ConsumerCase("c_16x16_b1_cb2", 1, 16, 16, 2, 1, seed=0),
    ConsumerCase("c_16x16_b3_cb2", 3, 16, 16, 2, 3, seed=10),
    ConsumerCase("c_32x32_b1_cb2", 1, 32, 32, 2, 1, seed=10),
    ConsumerCase("c_16x16_b1_cb3", 1, 16, 16, 3, 1, seed=0),
    ConsumerCase("c_16x16_b3_cb3", 3, 16, 16, 3, 3, seed=3),
    ConsumerCase("c_32x32_b1_cb3", 1, 32, 32, 3, 1, seed=2),
    ConsumerCase("c_32x32_b3_cb3", 3, 32, 32, 3, 3, seed=872),
    ConsumerCase("c_16x16_b257_cb1", 257, 16, 16, 1, 129, full=False),
]
C1 = 64


def consumer_inputs(c):
    rng = pp._rng(f"{c.name} main {c.seed}")
    x = rng.standard_normal((c.B, 1, c.H, c.W), dtype=np.float32)
    w1 = (rng.uniform(-1, 1, (C1, 1, 3, 3)) / 3.0).astype(np.float32)
    b1 = rng.uniform(-0.5, 0.5, C1).astype(np.float32)
    w2 = (rng.uniform(-1, 1, (pp.G8_COUT, C1, 3, 3)) / np.sqrt(9.0 * C1)).astype(np.float32)
    b2 = rng.uniform(-0.5, 0.5, pp.G8_COUT).astype(np.float32)
    z = lambda *s: np.zeros(s, np.float32)
    d1 = pp.stage_inputs(f"{c.name} 1 {c.seed}", pp.stage_of(CB[1], True), True, c.B, C1, c.H, c.W, y=z(c.B, C1, c.H, c.W))
    d2 = pp.stage_inputs(f"{c.name} 2 {c.seed}", c.stage, True, c.B, pp.G8_COUT, c.H, c.W, y=z(c.B, pp.G8_COUT, c.H, c.W))
    return x, w1, b1, w2, b2, d1, d2


def consumer_seed_ok(c, margin=2 * pp.MARGIN):
    """the consumer stage's max-pool decisions on the float64 chain from x: none within `margin` bounds (CPU only; the GPU test asserts MARGIN on the device's y)"""
    x, w1, b1, w2, b2, d1, d2 = consumer_inputs(c)
    conv = lambda t, w, b: cp.op64("fwd", cp._t(t), cp._t(w), w.shape).numpy() + b.astype(np.float64)[None, :, None, None]
    r1 = pp.forward64(pp.stage_of(CB[1], True), True, dict(d1, y=conv(x, w1, b1).astype(np.float32)), "tiles")
    r2 = pp.forward64(c.stage, True, dict(d2, y=conv(r1["out"].astype(np.float32), w2, b2).astype(np.float32)), "tiles")
    kd, pg = pp.conditioning(c.stage, r2)
    return kd >= margin and pg >= margin


def consumer_plans(c):
    """(producer Plan, consumer Plan) at p16_min_tiles = 1, from the mirror's own pieces: the producer as a G8Case's; the consumer's stage is `c.stage`"""
    g = pp.G8Case(c.name, c.B, C1, c.H, c.W, CB[1], ())
    p1, p2bare, _ = pp.g8_plans(g, 1)
    lean = pp.g8_plans(g, 1, guarded=False)[2]           # range_guard = 0: the producer's fp32 output is skipped
    assert p1.fwd == pp.F_G8 and p2bare.b == pp.B_G8, "the geometry must put the consumer's pass B on the operand-ready kernel"
    tiles2 = pp.conv_stat_tiles("f16x3", c.B, C1, pp.G8_COUT, c.H, c.W, in_p16=True)
    assert pp.post_g8_supported(pp.G8_COUT, c.H, c.W, c.stage.pool != "none", True)      # net.hip p16_dy_ok for the stage under test
    return p1, pp.plan(c.stage, True, c.B, pp.G8_COUT, c.H, c.W, "conv", tiles2, dy_p16=True), lean


@pytest.mark.parametrize("case", CONSUMER, ids=[c.name for c in CONSUMER])
def test_passb_combos_on_the_consumer_stage(ctx, case):
    import ganrev._lib as L
    from ganrev import nn
    x, w1, b1, w2, b2, d1, d2 = consumer_inputs(case)
    layers1, layers2 = CB[1], CB[case.combo]
    f1, f2 = pp.stage_of(layers1, True), case.stage
    Ho, Wo = (case.H // 2, case.W // 2) if f2.pool != "none" else (case.H, case.W)
    s1, s2 = (case.B, C1, case.H, case.W), (case.B, pp.G8_COUT, case.H, case.W)
    last1, conv2 = len(layers1), len(layers1) + 1
    first2 = conv2 + 1                                   # the consumer stage's first layer (its BatchNorm)
    gout = d2["gout"]
    p1, p2, lean = consumer_plans(case)
    assert p2.combo == case.combo and (p2.b, p2.nb) == (pp.B_G8, case.slices), p2.brief()
    prev = ctx.conv_mode()
    ctx.set_conv_mode("f16x3")
    seq = nn.Sequential().add(nn.SpatialConvolution(1, C1, 3, 3, 1, 1, 1, 1))
    for l in layers1:
        seq.add(tg._layer(l, C1))
    seq.add(nn.SpatialConvolution(C1, pp.G8_COUT, 3, 3, 1, 1, 1, 1))
    for l in layers2:
        seq.add(tg._layer(l, pp.G8_COUT))
    seq.training()
    try:
        ctx.set_tuning("p16_min_tiles", 1)
        seq.forward(x)
        net = seq._net
        net.set_params(np.concatenate([w1.ravel(), b1] + tg._stage_params(layers1, d1) + [w2.ravel(), b2] + tg._stage_params(layers2, d2)))

        def run(timed, skipped=False):
            net.set_bn_running(0, d1["rm0"], d1["rv0"])
            net.set_bn_running(1, d2["rm0"], d2["rv0"])
            tg._set_masks(net, layers1, d1, 1)
            tg._set_masks(net, layers2, d2, first2)
            c0 = tg._counts(ctx) if timed else None
            got = {"out": net.forward(x)}
            c1 = tg._counts(ctx) if timed else None
            got["y1"], got["y2"] = net.layer_output(0, s1), net.layer_output(conv2, s2)
            if skipped:
                with pytest.raises(L.GanrevError, match="operand-ready"):
                    net.layer_output(last1, s1)
            else:
                got["out1"] = net.layer_output(last1, s1)
            if f2.pool == "max":
                got["idx"] = net.pool_index(first2 + layers2.index("max"), case.B * pp.G8_COUT * Ho * Wo)
            net.zero_grads()
            got["gin"] = net.backward(x, gout)
            got["grads"] = net.get_grads()
            c2 = tg._counts(ctx) if timed else None
            return got, ((tg._delta(c1, c0), tg._delta(c2, c1)) if timed else None)

        got, again, (ran_fwd, ran_bwd) = tg._run_timed(ctx, run)
        ctx.set_tuning("range_guard", 0)
        try:
            lean_got, _ = run(False, skipped=lean)
        finally:
            ctx.set_tuning("range_guard", 1)
    finally:
        ctx.set_tuning("p16_min_tiles", 128)
        ctx.set_tuning("range_guard", 1)
        ctx.set_conv_mode(prev)
        if seq._net is not None:
            seq._net.close()
    add = lambda a, b: {k: a.get(k, 0) + b.get(k, 0) for k in set(a) | set(b)}
    want_bwd = dict(add(p1.bwd_labels(), p2.bwd_labels()), **{pp.BIAS: 1})
    assert ran_fwd == add(p1.fwd_labels(), p2.fwd_labels()), f"{case.name}: the forward launched {ran_fwd}"
    assert ran_bwd == want_bwd, f"{case.name}: the backward launched {ran_bwd}; post_paths predicts {want_bwd}"
    for k in got:
        assert np.array_equal(got[k], again[k]), f"{case.name} {k}: the timed pass differs from the untimed one"
    for k in lean_got:
        assert np.array_equal(lean_got[k], got[k]), f"{case.name} {k}: the lean run (range_guard 0) differs from the guarded one"
    # the guarded run against float64
    dd1, dd2 = dict(d1, y=got["y1"]), dict(d2, y=got["y2"])
    r1, r2 = pp.forward64(f1, True, dd1, "tiles"), pp.forward64(f2, True, dd2, "tiles")
    kink, pool = pp.violations(f2, r2)
    assert not kink.any() and (pool is None or not pool.any()), f"{case.name}: a decision of the consumer stage inside the margin on the device's y - choose another seed"
    ratios = {}

    def chk(key, val, ref, bound):
        ratios[key] = pp.check(np.asarray(val).reshape(np.shape(ref)), ref, bound, f"{case.name} {key}")

    chk("out", got["out"], r2["out"], r2["E_out"])
    if "idx" in got:
        assert np.array_equal(got["idx"], r2["idx"].reshape(-1)), f"{case.name}: pool_index() differs from the reference's argmax"
    bw2 = pp.backward64(f2, dd2, r2, bias=True)
    g = got["grads"]
    n1 = w1.size + C1 + sum(t.size for t in tg._stage_params(layers1, d1))
    o2 = n1 + w2.size
    chk("gbias2", g[o2:o2 + pp.G8_COUT], bw2["gbias"], bw2["E_gbias"])
    chk("ggamma2", g[o2 + pp.G8_COUT:o2 + 2 * pp.G8_COUT], bw2["ggamma"], bw2["E_ggamma"])
    chk("gbeta2", g[o2 + 2 * pp.G8_COUT:o2 + 3 * pp.G8_COUT], bw2["gbeta"], bw2["E_gbeta"])
    if case.full:
        refs2 = tg._main_grad_refs(types.SimpleNamespace(main="conv", C=pp.G8_COUT, B=case.B), got["out1"], w2, bw2["dy"], bw2["E_dy"], "f16x3")
        chk("gw2", g[n1:o2].reshape(w2.shape), *refs2["gw"])
        g1, Eg1 = refs2["gin"]
        bw1 = pp.backward64(f1, dd1, r1, gout=g1, Eg_in=Eg1, bias=True)
        o1 = w1.size
        chk("gbias1", g[o1:o1 + C1], bw1["gbias"], bw1["E_gbias"])
        st = tg._split_grads(layers1, g[o1 + C1:n1], C1)
        chk("ggamma1", st["ggamma"], bw1["ggamma"], bw1["E_ggamma"])
        chk("gbeta1", st["gbeta"], bw1["gbeta"], bw1["E_gbeta"])
        refs1 = tg._main_grad_refs(types.SimpleNamespace(main="conv", C=C1, B=case.B), x, w1, bw1["dy"], bw1["E_dy"], "f16x3")
        chk("gw1", g[:o1].reshape(w1.shape), *refs1["gw"])
        chk("gin", got["gin"], *refs1["gin"])
    print(f"{case.name}: max |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + f" [{p1.brief()} | {p2.brief()}]")


# ---------------------------------------------------------------- pass A: the single-round body and the one with the second buffer set
def passa_single_round(c):
    """elem.hip launch_post_backward: a block's batch slice is one round of 1024 float4 groups"""
    per = -(-c.B // pp.batch_splits(c.B * c.H * c.W, c.B))
    return per * (c.H * c.W // 4) <= 1024


PASSA = [
    # n = 12288 -> 3 slices of one 64 x 64 image: exactly 1024 groups, every slot of the batch loaded and used
    (pp.Case("one_round_exact_cb1", 3, 3, 64, 64, CB[1], "cb1 F:vec S:vec/3 A:vec/3 B:vec/3"), True),
    # n = 4096 -> one slice of four 32 x 32 images: 1024 groups across four images, pooled (combo 2), and combo 3's per-plane word
    (pp.Case("one_round_four_images_cb2", 4, 3, 32, 32, CB[2], "cb2 F:vec S:vec/1 A:vec/1 B:vec/1"), True),
    (pp.Case("one_round_four_images_cb3", 4, 3, 32, 32, CB[3], "cb3 F:vec S:vec/1 A:vec/1 B:vec/1"), True),
    # 640 groups: the last two slots of the batch are past the end
    (pp.Case("one_round_partial_cb1", 1, 5, 40, 64, CB[1], "cb1 F:vec S:vec/1 A:vec/1 B:vec/1"), True),
    (pp.BY_NAME["b29_21_to_15_slices"], False),                  # 1536 groups: a round and a half, the last slice one image (768)
    (pp.BY_NAME["three_rounds_last_partial"], False),            # combo 2, 1280 groups
]


@pytest.mark.parametrize("case,single", PASSA, ids=[c.name for c, _ in PASSA])
def test_passa_both_bodies(ctx, case, single):
    assert case.plan().brief() == case.expect and case.plan().a == pp.A_VEC
    assert passa_single_round(case) == single, "the case is about the other body of post_backward_a_vec_kernel"
    known = case.name in pp.BY_NAME
    if not known:
        pp.BY_NAME[case.name] = case          # pp.inputs() finds its cases by name; the table itself (CASES) is left alone
    try:
        tg.test_elementwise_stage_within_float64_bound(ctx, case)
    finally:
        if not known:
            del pp.BY_NAME[case.name]
