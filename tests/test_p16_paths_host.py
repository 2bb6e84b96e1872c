"""CPU checks of tests/p16_paths.py: the tables reach every operand-ready leaf and every edge, the hand-written expectations equal the restated
dispatch, every case is on the path its name claims, the restated a-priori bounds are upper bounds, and the error bound separates: CPU
emulations of the P16 arithmetic lie inside it (forward, data gradient, weight gradient; the image scaled 2^0, 2^4 and 2^7 above its tensor's
maximum), degraded ones put elements outside.  The evaluate() propagation accepts a float32 evaluation with P16 hand-overs and rejects
single-term hand-overs."""
import numpy as np
import pytest

import conv_paths as cp
import p16_paths as p16
import post_paths as pp

OVERSHOOT = (1.0, 16.0, 128.0)


def test_tables_reach_every_leaf_and_every_edge():
    reached = set()
    for c in p16.TRAIN_CASES:
        fwd, bwd = c.expect()
        reached |= set(fwd) | set(bwd)
    for c in p16.EVAL_CASES:
        reached |= set(c.on) & p16.P16_LEAVES
    assert reached == p16.P16_LEAVES, f"not reached: {sorted(p16.P16_LEAVES - reached)}; not a P16 leaf: {sorted(reached - p16.P16_LEAVES)}"
    cases = p16.TRAIN_CASES + p16.EVAL_CASES
    missing = [e for e, pred in p16.EDGES.items() if not any(pred(c, p16.route(c)) for c in cases)]
    assert not missing, f"edges no case reaches: {missing}"


@pytest.mark.parametrize("case", p16.TRAIN_CASES, ids=[c.name for c in p16.TRAIN_CASES])
def test_training_mirror_equals_expectation_and_case_is_on_its_path(case):
    assert case.mirror() == case.expect(), f"{case.name}: the restated dispatch gives {case.mirror()}, the table expects {case.expect()}"
    r = p16.train_route(case)
    H2, W2 = case.out_hw
    f = case.stage
    assert f.bn and f.act in ("ELU", "Sigmoid", "Tanh") and f.pool != "max", "producers without a discrete decision only"
    assert r.in_p16 and case.fwd in p16.P16_LEAVES
    assert pp.conv_p16_supported(case.B, case.C1, case.C2, H2, W2, 1) and pp.post_g8_supported(case.C1, case.H, case.W, f.pool != "none")
    assert r.p1.fwd == pp.F_G8 and r.p1.stats == "tiles" and r.p2.stats == "tiles"
    if not case.backward:
        return
    if any("quad" in k or "k32" in k for k in case.bwd):
        assert pp.conv_p16_supported(case.B, case.C2, case.C1, H2, W2, 1) and pp.post_g8_supported(case.C2, H2, W2, False, True)
        assert case.C2 % 16 == 0 and cp.round_up(case.C1, 32) % 64 == 0
    if p16.REDUCE_TILED in case.bwd:
        assert pp.conv_wgrad_p16_supported(case.B, case.C1, case.C2, H2, W2) and pp.post_g8_supported(case.C2, H2, W2, False, True)
        assert p16.train_route(case, guarded=False).lean, "a case with the P16 weight gradient skips the producer's fp32 output when lean"
    assert (r.p2.b == pp.B_G8) == bool(case.bwd), "the g8 pass B writes the dy image exactly where a P16 gradient kernel reads it"
    # at the library's default p16_min_tiles the small cases are not operand-ready at all: the tuning key is what puts them on the path
    assert p16.train_route(case, min_tiles=128).in_p16 == pp.conv_p16_supported(case.B, case.C1, case.C2, H2, W2, 128)


@pytest.mark.parametrize("case", p16.EVAL_CASES, ids=[c.name for c in p16.EVAL_CASES])
def test_evaluate_mirror_equals_expectation_and_case_is_on_its_path(case):
    assert case.mirror(1) == case.on, f"{case.name}: eval_p16 = 1: the restated dispatch gives {case.mirror(1)}"
    assert case.mirror(0) == case.off, f"{case.name}: eval_p16 = 0: the restated dispatch gives {case.mirror(0)}"
    assert not any("_po" in k or "p16o" in k or k in p16.P16_LEAVES for k in case.off)
    r = p16.eval_route(case)
    st = case.stages()
    assert r[0]["po"] and case.on[0] == p16.fewin_p16o_label(case.c0)
    for i in range(1, len(st)):
        cin, co, h, w, _, pool = st[i]
        assert r[i]["in_p16"] and pp.conv_p16_supported(case.B, cin, co, h, w, 1)
        if i + 1 < len(st):
            assert r[i]["po"] != r[i]["post_p16"] and r[i]["post_p16"] == pool
            assert not pool or pp.post_g8_supported(co, h, w, True)


def test_weight_gradient_block_numbering_is_a_bijection():
    """both numberings of wgrad_p16_block deal every (cb, ob, split) exactly once, and the same-XCD numbering keeps a split's combinations 8 ids apart"""
    seen = set()
    for c in p16.TRAIN_CASES:
        g = p16.train_route(c).wgrad
        if g is None or not c.backward:
            continue
        ids = [p16.wgrad_p16_block(g["n_cb"], g["n_ob"], g["nsplit"], bid) for bid in range(g["grid"])]
        want = {(cb, ob, s) for cb in range(g["n_cb"]) for ob in range(g["n_ob"]) for s in range(g["nsplit"])}
        assert len(ids) == len(set(ids)) and set(ids) == want, c.name
        assert sum(a + b for a, b in g["runs"]) == g["units"] and all(a >= b and a - b <= 1 for a, b in g["runs"]), c.name
        if g["xcd"]:
            by_split = {}
            for bid, (_, _, s) in enumerate(ids):
                by_split.setdefault(s, []).append(bid)
            assert all(len({b % 8 for b in v}) == 1 for v in by_split.values()), c.name
        seen.add(g["xcd"])
    assert seen == {True, False}


def test_fewin_output_channel_slices():
    """`og` by hand: 48 channels -> two slices of 24 (a third doubling would split an 8-channel group pair: 48 % 32 != 0); 64 -> eight of 8;
    16 channels are halved unless the grid alone reaches 1024 workgroups"""
    assert p16.fewin_og(3, 48, True) == 2 and p16.fewin_og(4, 64, True) == 8 and p16.fewin_og(3, 16, True) == 2
    assert p16.fewin_og(1024, 16, True) == 1 and p16.fewin_og(1023, 16, True) == 2 and p16.fewin_og(3, 24, True) == 1
    assert p16.fewin_og(3, 48, False) == 4 and p16.fewin_og(3, 24, False) == 2 and p16.fewin_og(600, 64, False) == 2      # fp32 output: any 8 channels


def test_training_references_hold_no_discrete_decision():
    """ELU, Sigmoid, Tanh and the average pool: post_paths.violations finds nothing to condition on the float64 reference, so nothing is
    excluded from any comparison (the cap on excluded elements is zero)"""
    for c in p16.TRAIN_CASES:
        assert c.stage.act not in pp.KINK and c.stage.pool != "max"
    c = p16.TRAIN_BY_NAME["k32_behind_avg_pool"]
    x, w1, b1, _, _, d1, _ = p16.train_inputs(c)
    y1 = cp.op64("fwd", cp._t(x), cp._t(w1), w1.shape).numpy() + b1.astype(np.float64)[None, :, None, None]
    r = pp.forward64(c.stage, True, dict(d1, y=y1), "tiles")
    kink, pool = pp.violations(c.stage, r)
    assert not kink.any() and pool is None


# ---------------------------------------------------------------- the a-priori bounds are upper bounds
@pytest.mark.parametrize("name", ["k32_one_chunk_ragged_xcd", "k32_behind_avg_pool", "quad32_tiles_y2_padded_out", "k32_three_chunks_padded_out"])
def test_restated_bounds_are_upper_bounds_of_their_tensors(name):
    c = p16.TRAIN_BY_NAME[name]
    x, w1, b1, w2, b2, d1, d2 = p16.train_inputs(c)
    y1 = cp.op64("fwd", cp._t(x), cp._t(w1), w1.shape).numpy() + b1.astype(np.float64)[None, :, None, None]
    r1 = pp.forward64(c.stage, True, dict(d1, y=y1), "tiles")
    Bd = p16.bound_fwd(c.stage, y1, d1["gamma"], d1["beta"])
    top = float(np.abs(r1["out"]).max())
    print(f"{name}: max|out1| {top:.3f}, Bd {Bd:.3f} (x{Bd / top:.2f})")
    assert top <= Bd <= 64 * top
    y2 = cp.op64("fwd", cp._t(r1["out"]), cp._t(w2), w2.shape).numpy() + b2.astype(np.float64)[None, :, None, None]
    f2 = pp.Stage(bn=True)
    dd2 = dict(d2, y=y2)
    r2 = pp.forward64(f2, True, dd2, "tiles")
    bw2 = pp.backward64(f2, dd2, r2)
    Bdy = p16.bound_dy(y2, d2["gamma"], np.abs(bw2["dz"]).max())
    top = float(np.abs(bw2["dy"]).max())
    print(f"{name}: max|dy2| {top:.3e}, Bd {Bdy:.3e} (x{Bdy / top:.2f})")
    assert top <= Bdy <= 4096 * top


# ---------------------------------------------------------------- the bound separates
SEPARATE = [("fwd", "quad16_three_chunks_cout100"), ("fwd", "k32_three_chunks_padded_out"), ("fwd", "quad32_tiles_y2_padded_out"),
            ("dgrad", "dgrad_quad16_padded_48_48"), ("dgrad", "quad32_tiles_x2"), ("wgrad", "wgrad16_plain_numbering_two_blocks"),
            ("wgrad", "wgrad32_non_square")]


@pytest.mark.parametrize("op,name", SEPARATE, ids=[f"{o}-{n}" for o, n in SEPARATE])
def test_bound_accepts_the_p16_arithmetic_and_rejects_degraded(op, name):
    c = p16.TRAIN_BY_NAME[name]
    H2, W2 = c.out_hw
    rng = pp._rng(f"{name} {op} separate")
    x = rng.standard_normal((c.B, c.C1, H2, W2)).astype(np.float32)
    w = (rng.uniform(-1, 1, (c.C2, c.C1, 3, 3)) / np.sqrt(9.0 * c.C1)).astype(np.float32)
    dy = (0.1 * rng.standard_normal((c.B, c.C2, H2, W2))).astype(np.float32)
    a, b = (x, w) if op == "fwd" else (dy, w) if op == "dgrad" else (x, dy)
    for over in OVERSHOOT:
        a_mag = float(np.abs(a).max()) * over
        b_mag = float(np.abs(b).max()) * (over if op == "wgrad" else 1.0)          # weights: their own maximum; dy in a weight gradient: an image too
        ref, bound = p16.conv_ref(op, x, w, None, dy, a_scale=a_mag, b_scale=b_mag if op == "wgrad" else None)
        got = p16.emulate_conv("p16", op, a, b, w.shape, a_mag, b_mag)
        ratio = cp.check_bound(got, ref, bound, f"{name} {op} P16 emulation, image scaled x{over:g} above its maximum")
        print(f"{name} {op} overshoot x{over:g}: max |err| / bound {ratio:.3f}")
        for kind in ("without_x1w0", "without_x0w1", "single_term", "last_chunk_left_out"):
            bad = p16.emulate_conv(kind, op, a, b, w.shape, a_mag, b_mag)
            outside = int((np.abs(bad.astype(np.float64) - ref) > bound).sum())
            assert outside >= 1, f"{name} {op} x{over:g}: the bound accepts the emulation {kind}"


def test_bound_at_the_tensor_maximum_is_the_default_bound():
    """a_scale = max|a| reproduces conv_paths.reference's default: the new argument changes nothing for existing callers"""
    c = p16.TRAIN_BY_NAME["quad16_one_chunk"]
    rng = pp._rng("default bound")
    x = rng.standard_normal((c.B, c.C1, 16, 16)).astype(np.float32)
    w = rng.uniform(-1, 1, (c.C2, c.C1, 3, 3)).astype(np.float32)
    r0, b0 = p16.conv_ref("fwd", x, w, None, None)
    r1, b1 = p16.conv_ref("fwd", x, w, None, None, a_scale=float(np.abs(x).max()), b_scale=float(np.abs(w).max()))
    r2, b2 = p16.conv_ref("fwd", x, w, None, None, a_scale=16 * float(np.abs(x).max()))
    assert np.array_equal(r0, r1) and np.array_equal(b0, b1) and np.array_equal(r0, r2) and (b2 > b0).all()


# (name, the hand-over is rejected at the net output; False: only at the pooling stage's raw output - eval_chain's HOW TIGHT)
PROPAGATE = [("fewin2_og2_o_per24", True), ("fewin3_og8_two_tile_rows", True), ("po16_c48_c40", True), ("po32_c48_c40", True), ("post_p16_avg_pool", False)]


@pytest.mark.parametrize("name,at_output", PROPAGATE, ids=[n for n, _ in PROPAGATE])
def test_evaluate_propagation_accepts_p16_handover_and_rejects_single_term(name, at_output):
    c = p16.EVAL_BY_NAME[name]
    x, params = p16.eval_inputs(name)
    ref, E, bds, raws = p16.eval_chain(c, x, params)
    assert len(bds) == len(c.C) - 1 and all(b > 0 for b in bds)
    got, got_raw = p16.emulate_eval32(c, x, params, bds)
    ratio = pp.check(got, ref, E, f"{name}: float32 chain with P16 hand-overs")
    print(f"{name}: float32 chain with P16 hand-overs, max |err| / bound {ratio:.3f}; Bd {', '.join(f'{b:.3g}' for b in bds)}")
    bad, bad_raw = p16.emulate_eval32(c, x, params, bds, terms=1)
    print(f"{name}: single-term hand-overs, max |err| / bound {pp.worst_ratio(bad, ref, E):.2f} at the output")
    if at_output:
        assert (np.abs(bad.astype(np.float64) - ref) > E).any(), f"{name}: the propagated bound accepts a single-term hand-over"
    for i, (_, _, _, _, _, pool) in enumerate(c.stages()):
        if pool:         # the raw output of a stage without a fused epilogue is observable (layer_output): one hand-over behind it
            y, Ey = raws[i]
            pp.check(got_raw[i], y, Ey, f"{name}: stage {i} raw output, P16 hand-over")
            assert (np.abs(bad_raw[i].astype(np.float64) - y) > Ey).any(), f"{name}: stage {i} raw output: the bound accepts a single-term hand-over"
    assert at_output or any(s[5] for s in c.stages())
