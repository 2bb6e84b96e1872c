"""CPU checks of tests/post_paths.py: the case table reaches every combination the restated pipeline dispatch reaches on a grid of shapes, every
hand-written expectation equals the mirror, the mirror names no label outside LABELS, post_combo and post_specialize agree, every case's inputs
are conditioned (no decision a rounding could turn, nothing excluded), and the per-element float64 bound accepts a float32 emulation in the
kernels' operation order while rejecting each subtly degraded one by a stated factor."""
import itertools
import math

import numpy as np
import pytest

import post_paths as pp

ELEM = [c for c in pp.CASES if c.main == "elem"]
GRID_H = (2, 4, 6, 7, 8, 9, 12, 16, 17)
GRID_W = (4, 6, 7, 8, 9, 12, 16, 20, 24)
GRID_B = (1, 3)
REACHED = (68, 12, 7)   # combinations (main x forward label x statistics route x pass A x pass B x combo x pool x mask kinds x BatchNorm): element-wise; convolution + one stage; the operand-ready producer / consumer pairs


def _keys(cases):
    return {c.plan().key(c.stage, c.main) for c in cases}


def test_every_expectation_equals_the_mirror():
    assert len(pp.BY_NAME) == len(pp.CASES), "case names are unique"
    for c in pp.CASES + [pp.NT_CASE]:
        assert c.plan().brief() == c.expect, (c.name, c.plan().brief(), c.expect)
    for c in pp.G8_CASES:
        p1, p2, lean = pp.g8_plans(c, 1, guarded=False)
        assert (p1.brief(), p2.brief(), "lean" if lean else "kept") == c.expect, (c.name, p1.brief(), p2.brief(), lean)
        assert not pp.g8_plans(c, 1, guarded=True)[2], "a range-guarded call keeps every fp32 tensor"
    for name, layers, training, combo in pp.FORMS:
        assert pp.post_combo(pp.stage_of(layers, training)) == combo, name
    assert {cb for _, _, _, cb in pp.FORMS} == set(range(12)), "every specialisation 1..11 and the generic kernel"
    assert {cb for _, _, tr, cb in pp.FORMS if not tr} >= {10, 11}


def test_case_table_reaches_every_combination_of_the_grid():
    """Every stage form of the table, on every plane of the grid, in element-wise nets: the combinations the mirror produces there are exactly
    the table's element-wise ones.  The main-operator cases add the tile statistics, the bias job and the statistics pass behind a convolution."""
    reachable = {}
    for (_, layers, training, _), H, W, B in itertools.product(pp.FORMS, GRID_H, GRID_W, GRID_B):
        f = pp.stage_of(layers, training)
        if f.pool != "none" and (H < 2 or W < 2):
            continue
        reachable.setdefault(pp.plan(f, training, B, 5, H, W).key(f, "elem"), (layers, training, B, H, W))
    table = _keys(ELEM)
    missing = sorted(set(reachable) - table, key=str)
    assert not missing, [(k, reachable[k]) for k in missing]
    assert table <= set(reachable), sorted(table - set(reachable), key=str)
    # convolution + one stage: every form of the table's conv cases, on every plane of the grid, behind a few-input convolution (tiles) and
    # behind a 4-plane one (the statistics pass)
    conv = [c for c in pp.CASES if c.main == "conv" and c.depth == 1]
    reach_conv = {}
    for layers, H, W, B, cin in itertools.product(sorted({c.layers for c in conv}), GRID_H, GRID_W, GRID_B, (3, 4)):
        f = pp.stage_of(layers, True)
        tiles = pp.conv_stat_tiles("f32", B, cin, 5, H, W)
        reach_conv.setdefault(pp.plan(f, True, B, 5, H, W, "conv", tiles).key(f, "conv"), (layers, B, cin, H, W))
    table_conv = _keys(conv)
    assert not set(reach_conv) - table_conv, [(k, reach_conv[k]) for k in sorted(set(reach_conv) - table_conv, key=str)]
    assert table_conv <= set(reach_conv)
    # the operand-ready pairs: every producer form of the g8 table, at every g8 plane, 16 and 64 producer channels, B 1, 3 and 257, with the
    # P16 path forced (p16_min_tiles 1); both stages' combinations
    reach_g8 = {}
    for layers, HW, B, C1 in itertools.product(sorted({c.layers for c in pp.G8_CASES}), (16, 32, 64), (1, 3, 257), (16, 64)):
        c = pp.G8Case("grid", B, C1, HW, HW, layers, ())
        if c.stage.pool != "none" and HW != 32:
            continue                       # (a pool from 16 x 16 leaves 8 x 8: no P16 consumer; from 64 x 64: 32 x 32, as no pool at 32 x 32)
        p1, p2, _ = pp.g8_plans(c, 1)
        reach_g8.setdefault(p1.key(c.stage, "conv"), (layers, B, C1, HW))
        reach_g8.setdefault(p2.key(pp.Stage(bn=True), "conv"), (layers, B, C1, HW))
    table_g8 = set()
    for c in pp.G8_CASES:
        p1, p2, _ = pp.g8_plans(c, 1)
        table_g8 |= {p1.key(c.stage, "conv"), p2.key(pp.Stage(bn=True), "conv")}
    assert not set(reach_g8) - table_g8, [(k, reach_g8[k]) for k in sorted(set(reach_g8) - table_g8, key=str)]
    assert table_g8 <= set(reach_g8)
    assert any(k[1] == pp.F_G8 for k in table_g8) and any(k[4] == pp.B_G8 for k in table_g8)
    print(f"combinations on the grids and in the table: {len(table)} element-wise, {len(table_conv)} convolution + stage, {len(table_g8)} operand-ready")
    assert (len(table), len(table_conv), len(table_g8)) == REACHED
    main = [c for c in pp.CASES if c.main != "elem"]
    assert {c.plan().stats for c in main} >= {"tiles", "none", pp.S_VEC, pp.S_SCALAR}
    assert any(c.plan().bias and c.depth > 16 for c in main), "more bias jobs than one launch takes"
    assert any(not c.stage.bn and c.stage.act == "Sigmoid" for c in main) and any(not c.stage.bn and c.stage.act == "PReLU" for c in main)
    assert any(c.main == "linear" and (c.B, c.C, c.H, c.W) == (5, 37, 1, 1) for c in main)


def test_mirror_names_no_label_outside_the_closed_set():
    for (_, layers, training, _), H, W, B in itertools.product(pp.FORMS, GRID_H + (32, 64), GRID_W + (32, 64), GRID_B + (29, 300)):
        f = pp.stage_of(layers, training)
        pool = f.pool != "none"
        for main, tiles, C in (("elem", 0, 5), ("conv", 0, 8), ("conv", 3, 8), ("linear", 0, 8)):
            for g8 in (False, True):
                if g8 and not (f.bn and main == "conv" and pp.post_g8_supported(C, H, W, pool) and pp.post_g8_supported(C, H, W, pool, True)):
                    continue
                p = pp.plan(f, training, B, C, H, W, main, tiles, p16_out=g8, dy_p16=g8)
                assert set(p.fwd_labels()) | set(p.bwd_labels()) <= pp.LABELS, p
                assert (p.b == pp.B_G8) == (g8 and training and pp.bwd_vec(pool, B, C, H, W))
    assert pp.BIAS in pp.LABELS and pp.bias_launches(17) == 2 and pp.bias_launches(16) == 1 and pp.bias_launches(0) == 0


def test_post_combo_and_post_specialize_agree():
    """post_combo picks CB from the stage description, post_specialize<CB> overwrites the description with constants: the constants of CB must be
    the one description that post_combo maps to CB - otherwise the kernel silently computes another stage.  Both sides here are RESTATEMENTS
    (post_paths.post_combo, post_paths.SPECIALIZED): this holds the two restated tables to each other; what holds elem.hip's own
    post_specialize<CB> is the per-combo value cases of tests/test_gpu_post_paths.py on the float4 route."""
    seen = {}
    for bn, act, m1, pool, m2 in itertools.product((False, True), pp.ACTS, ("none", "elem", "spatial", "scale"), ("none", "max", "avg"),
                                                   ("none", "elem", "spatial", "scale")):
        f = pp.Stage(bn, act, m1, pool, m2)
        cb = pp.post_combo(f)
        if cb:
            assert cb not in seen, f"combo {cb}: {seen[cb]} and {f}"
            seen[cb] = f
    assert seen == pp.SPECIALIZED


def test_split_rules():
    n = 29 * 48 * 64
    assert pp.stat_splits(n) == 21 and pp.batch_splits(n, 29) == 15, "the B = 29 fault: 21 requested slices, 15 that own an image"
    assert pp.batch_splits(128 * 64 * 64, 128) == pp.STAT_SPLITS
    for B, hw in itertools.product(range(1, 140), (16, 64, 96, 3072, 4096)):
        s = pp.batch_splits(B * hw, B)
        per = -(-B // s)
        assert 1 <= s <= min(B, pp.STAT_SPLITS) and (s - 1) * per < B <= s * per, (B, hw, s)
    for B in (1, 7, 256, 257, 300, 513):
        s = pp.g8_slices(B)
        per = -(-B // s)
        assert s <= pp.PB_SPLITS and (s - 1) * per < B <= s * per
    assert pp.g8_slices(300) == 150 and pp.g8_slices(256) == 256
    assert pp.post_g8_supported(16, 16, 16, False) and pp.post_g8_supported(64, 32, 32, True) and pp.post_g8_supported(64, 64, 64, False, True)
    assert not pp.post_g8_supported(12, 16, 16, False) and not pp.post_g8_supported(16, 8, 12, True) and not pp.post_g8_supported(16, 48, 32, False)
    assert pp.post_g8_supported(16, 16, 32, True, True) and not pp.post_g8_supported(16, 16, 32, True), "backward: the pre-pool plane counts"
    assert pp.g8_blocks(3, 16, 16, 16, False) == 6 and pp.g8_blocks(3, 16, 32, 32, False) == 24 and pp.g8_blocks(3, 16, 64, 64, False) == 96
    assert pp.post_big(32, 64, 128, 128) and not pp.post_big(32, 64, 128, 124)
    by = pp.BY_NAME
    assert [by[k].tiles for k in ("conv_tiles_3", "conv_tiles_66", "conv_tiles_520", "conv_pass_cin4")] == [3, 66, 520, 0]
    assert pp.conv_stat_tiles("f16x3", 8, 64, 64, 32, 32) == 0 and pp.conv_stat_tiles("f16x3", 128, 64, 64, 32, 32) == 256
    assert pp.conv_stat_tiles("f32", 128, 64, 64, 32, 32) == 0 and pp.conv_stat_tiles("bf16x6", 3, 3, 300, 16, 16) == 0
    assert pp.stats_route(pp.Stage(bn=True), True, "linear", 5) == "pass" and pp.stats_route(pp.Stage(bn=True), False, "conv", 5) == "eval"


def test_cases_sit_on_the_edges():
    cs = {c.name: c for c in pp.CASES}
    assert {c.C % 4 for c in ELEM} >= {1, 2, 3}, "channel counts off the four-channels-per-workgroup kernels"
    assert any(c.H % 2 and c.W % 2 and c.stage.pool == "max" for c in ELEM) and any(c.H % 2 and c.stage.pool == "avg" for c in ELEM), "floor rule"
    groups = lambda c: c.H * c.W // 4
    assert any(groups(c) & (groups(c) - 1) for c in ELEM if c.plan().a == pp.A_VEC), "udivp's division branch"
    c = cs["b29_21_to_15_slices"]
    per = -(-c.B // c.plan().na)
    assert per * groups(c) > 1024 and (per * groups(c)) % 1024, "several prefetch rounds, the last partial"
    assert c.B % per, "a shorter last slice"
    c = cs["stat_splits_cap_b128"]
    assert c.plan().na == pp.STAT_SPLITS and c.B // c.plan().na == 2
    c = cs["slice_below_256_groups"]
    assert c.B * groups(c) < 256
    g8 = pp.G8_BY_NAME
    assert {(c.H, c.stage.pool) for c in pp.G8_CASES} >= {(16, "none"), (32, "max"), (32, "avg"), (32, "none"), (64, "none")}
    assert any(c.B % 2 for c in pp.G8_CASES) and pp.g8_plans(g8["g8_b257_two_images_per_slice"], 1)[1].nb == 129, "B > 256: two images per slice"
    assert pp.g8_blocks(3, 64, 32, 32, False) == 4 * 3 * 8 and pp.g8_blocks(3, 64, 16, 16, False) == 3 * 8, "the blocks *= 4 branch"
    assert pp.post_big(pp.NT_CASE.B, pp.NT_CASE.C, pp.NT_CASE.H, pp.NT_CASE.W) and 4 * pp.NT_CASE.B * pp.NT_CASE.C * pp.NT_CASE.H * pp.NT_CASE.W == 128 << 20
    assert cs["scalar_splits_3"].plan().nstat == 3 and (cs["scalar_splits_3"].H * cs["scalar_splits_3"].W) % 4


@pytest.mark.parametrize("case", ELEM, ids=[c.name for c in ELEM])
def test_inputs_are_conditioned(case):
    d, _ = pp.inputs(case.name)
    f = case.stage
    r = pp.forward64(f, case.training, d)
    kink, pool = pp.violations(f, r)
    kd, pg = pp.conditioning(f, r)
    assert not kink.any() and (pool is None or not pool.any()), "elements a test would have to exclude: must be zero"
    assert kd >= pp.MARGIN and pg >= pp.MARGIN, (kd, pg)
    if f.bn:
        assert (d["gamma"] > 0).any() and (d["gamma"] < 0).any() and (d["gamma"] == 0).sum() == 1
        if case.training:
            off = np.abs(d["y"].astype(np.float64).mean((0, 2, 3))) / d["y"].astype(np.float64).std((0, 2, 3))
            assert off.max() > 20 and off.min() < 2, "channel offsets from 0 to 32 spreads"


def test_bound_accepts_the_float32_emulation():
    worst = {}
    for c in ELEM:
        d, _ = pp.inputs(c.name)
        obs, idx, _, _ = pp.observables(c.stage, c.training, d)
        em = pp.emulate(c.stage, c.training, d)
        if idx is not None:
            assert np.array_equal(em["idx"], idx), c.name
        for k, (ref, bound) in obs.items():
            w = pp.check(em[k], ref, bound, f"{c.name} {k}")
            if w > worst.get(k, (0, ""))[0]:
                worst[k] = (w, c.name)
    print("float32 emulation, max |err| / bound: " + ", ".join(f"{k} {w:.3f} ({n})" for k, (w, n) in worst.items()))
    assert set(worst) == {"out", "run_mean", "run_var", "dy", "ggamma", "gbeta", "gslope"}


# (case, degradation, observable that must leave its bound, by at least this factor; MEASURED factor in the comment)
DEGRADED = [
    ("cb1_6x16", "mask_shift", "dy", 1e4, {}),                               # 7e6; the output holds elements that must be exactly 0
    ("cb2_6x16", "mask_shift", "gbeta", 1e4, {}),                            # 1e6 (mask 2, behind the pool)
    ("cb3_6x16", "mask_shift", "ggamma", 1e4, {}),                           # 9e5 (the spatial mask)
    ("b29_21_to_15_slices", "drop_last_slice", "run_mean", 1e4, {"nslices": 15}),   # 5e5
    ("b29_21_to_15_slices", "fp32_stats", "out", 100, {}),                   # 929
    ("stat_splits_cap_b128", "fp32_stats", "run_mean", 50, {}),              # 221
    ("cb8_6x16", "fp32_stats", "run_var", 100, {}),                          # 1176: 288 elements are enough
    ("cb8_6x16", "biased_running_var", "run_var", 1000, {}),                 # 11158
    ("b29_21_to_15_slices", "biased_running_var", "run_var", 10, {}),        # 62 at n = 89088
    ("cb8_6x16", "no_eps", "out", 10, {}),                                   # 52
    ("cb10_6x16", "no_eps", "out", 4, {}),                                   # 10 (evaluate(): the running variance)
    ("drop_avg_drop_6x16", "avg_no_quarter", "dy", 1e4, {}),                 # 2.5e7
    ("bn_relu_avg_9x7", "avg_no_quarter", "ggamma", 1e4, {}),                # 2.7e6
    ("cb1_6x16", "no_k", "dy", 1e4, {}),                                     # 2.4e5
    ("cb10_6x16", "combo_neighbour", "out", 1e4, {}),                        # 4e6: the stage of combo 11 computed for combo 10
    ("cb11_6x16", "combo_neighbour", "out", 1e4, {}),                        # 3e6
]


@pytest.mark.parametrize("name,wrong,key,factor,kw", DEGRADED, ids=[f"{n}-{w}" for n, w, _, _, _ in DEGRADED])
def test_bound_rejects_degraded_emulations(name, wrong, key, factor, kw):
    c = pp.BY_NAME[name]
    d, _ = pp.inputs(name)
    obs, _, _, _ = pp.observables(c.stage, c.training, d)
    em = pp.emulate(c.stage, c.training, d, wrong=wrong, **kw)
    w = pp.worst_ratio(em[key], *obs[key])
    print(f"{name} {wrong}: {key} at {w:.3g} x its bound")
    assert w >= factor


def test_activation_constants_are_twice_the_measured():
    for act in ("Sigmoid", "Tanh"):
        m = 0.0
        for c in ELEM:
            if c.stage.act != act:
                continue
            d, _ = pp.inputs(c.name)
            z32 = pp.forward64(c.stage, c.training, d)["z"].astype(np.float32)
            a64 = pp.act64(act, z32.astype(np.float64), 0.0)
            m = max(m, float((np.abs(pp._act32(act, z32, np.float32(0)).astype(np.float64) - a64) / (pp.U * np.abs(a64))).max()))
        print(f"{act}: float32 numpy against float64, max |err| / (U |a|) = {m:.2f}; C_ACT {pp.C_ACT[act]}")
        assert pp.C_ACT[act] == math.ceil(2 * m)
    # ELU's negative branch: float32 numpy expf - 1 against float64, absolute (the device's hardware exponential: elem.hip documents 3e-7)
    z = np.linspace(-30, 0, 200001).astype(np.float32)
    e = float(np.abs((np.exp(z) - np.float32(1)).astype(np.float64) - np.expm1(z.astype(np.float64))).max())
    print(f"ELU z <= 0: float32 numpy max abs error {e:.2e}; bound ELU_ABS + U = {pp.ELU_ABS + pp.U:.2e}")
    assert e <= pp.ELU_ABS + pp.U
