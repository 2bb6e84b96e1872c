"""CPU checks of tests/gemm_paths.py: the case table reaches every leaf of the restated nn.Linear GEMM dispatch at the shapes where kernels go
wrong, the mirror names nothing a net cannot reach, the workspace rule covers every plan, and the per-element float64 bound accepts correct
emulations of the fp32 and f16x3 GEMMs while rejecting subtly degraded ones."""
import numpy as np
import pytest

import gemm_paths as gp

GRID_B = (1, 3, 5, 33, 64, 70, 128, 129, 130, 160, 256, 257, 300, 512, 1153, 2048)
GRID_DIMS = (1, 2, 5, 7, 8, 24, 36, 40, 64, 65, 100, 102, 127, 128, 130, 256, 301, 512, 640, 1024, 1030, 1056, 1100, 2052, 4096, 8192, 8200,
             10300, 10500)
MAX_WEIGHTS = 1.4e6      # the table's limit per weight matrix


def _grid():
    for mode in ("f32", "f16x3"):          # (bf16x6: the fp32 kernel, as f32)
        for B in GRID_B:
            for nin in GRID_DIMS:
                for nout in GRID_DIMS:
                    for post in (False, True):
                        yield mode, B, nin, nout, post


def _case_launches():
    return [(c, op, l) for c in gp.CASES for op, l in c.launches().items()]


def test_case_table_reaches_every_fork():
    """Each case's hand-written expectation equals the mirror; together the cases hold every combination (Launch.combo: kernel x split x
    A load x B load x store paths x accumulate x bias place x epilogue) that any shape of the grid with a weight matrix within the table's
    limit reaches - 1-wide layers included - with none left out."""
    assert len(gp.BY_NAME) == len(gp.CASES), "case names are unique"
    for c in gp.CASES:
        assert c.nin * c.nout <= MAX_WEIGHTS, c.name
        got = tuple(c.launches()[op].brief() for op in c.ops)
        assert got == c.expect, (c.name, got, c.expect)
    table = {l.combo() for _, _, l in _case_launches()}
    reachable = {}
    for mode, B, nin, nout, post in _grid():
        if nin * nout > MAX_WEIGHTS:
            continue
        l = gp.linear_launches(mode, B, nin, nout, post, training=not post)
        for op in (("fwd",) if post else gp.OPS):
            reachable.setdefault(l[op].combo(), []).append((mode, B, nin, nout, post, op))
    missing = sorted(set(reachable) - table, key=str)
    assert not missing, [(f, reachable[f][0]) for f in missing]
    assert table <= set(reachable), "the grid is wide enough to reach what the table reaches"
    print(f"{len(reachable)} leaves reachable on the grid, {len(table)} in the table")
    assert {f[0] for f in table} == {gp.MFMA, gp.F16X3, gp.BIG}
    assert {c.mode for c in gp.CASES} == {"f32", "bf16x6", "f16x3"}
    assert {c.act for c in gp.CASES if c.post} == set(gp.ACTS) and any(c.post and not c.bn for c in gp.CASES)
    assert any(c.mode == "f16x3" and not c.f16 and c.nin * c.nout == gp.F16_MIN_WEIGHTS - 1 for c in gp.CASES), "one weight below the f16x3 threshold"
    assert any(c.f16 and c.nin * c.nout == gp.F16_MIN_WEIGHTS for c in gp.CASES), "exactly at the f16x3 threshold"


def test_cases_sit_on_the_edges():
    """Per kernel: a partial tile in M and in N, a K that is no multiple of the 32-wide chunk and one that is no multiple of 4; split counts
    of at least 8 (the reduce's unrolled loop) and off a multiple of 8; a last K run shorter than klen; both store paths in one launch of
    the 128-tile kernel; a fall-back from the 128-tile plan."""
    ls = _case_launches()
    for kernel, tile in ((gp.MFMA, 64), (gp.F16X3, 64), (gp.BIG, 128)):
        dims = [c.dims(op) for c, op, l in ls if l.kernel == kernel]
        assert any(M % tile for M, N, K in dims) and any(N % tile for M, N, K in dims), kernel
        assert any(K % 32 for M, N, K in dims) and any(K % 4 for M, N, K in dims), kernel
        assert kernel == gp.F16X3 or any(K < 32 for M, N, K in dims), f"{kernel}: a K below one chunk"
        assert {M % 32 for M, N, K in dims} >= {27, 31}, f"{kernel}: rows ending one short of a lane half's last row (gemm_store_block's `full`)"
        assert any(l.nsplit >= 8 for c, op, l in ls if l.kernel == kernel), kernel
        assert any(l.nsplit > 1 and l.nsplit % 8 for c, op, l in ls if l.kernel == kernel), kernel
        assert any(l.nsplit > 1 and c.dims(op)[2] % l.klen for c, op, l in ls if l.kernel == kernel), f"{kernel}: a short last K run"
        assert any(l.nsplit > 1 and (c.dims(op)[2] % l.klen) % 32 for c, op, l in ls if l.kernel == kernel), f"{kernel}: a ragged chunk in the last K run"
    assert any(l.kernel == gp.BIG and l.store == {"vec", "scalar"} and l.nsplit == 1 for c, op, l in ls)
    assert any(l.kernel == gp.BIG and l.store == {"vec", "scalar"} and l.nsplit > 1 for c, op, l in ls)
    assert any(l.kernel == gp.BIG and l.store == {"vec", "scalar"} and l.epilogue == "fused" for c, op, l in ls)
    assert any(l.nsplit > 1 and l.accumulate for c, op, l in ls), "the reduce accumulating onto gw0"
    fell_back = [(c.name, op) for c, op, l in ls if c.f16 and l.kernel == gp.F16X3 and min(c.dims(op)[:2]) >= 128]
    assert {op for _, op in fell_back} >= {"fwd", "wgrad"}, fell_back
    assert any(c.dims(op)[2] == 257 for c, op, l in ls if (c.name, op) in fell_back)


def test_mirror_on_a_grid():
    """Over a grid of (mode, B, nin, nout), with and without an evaluate()-mode epilogue: only the four labels; never the
    <AK = false, BK = true> kernels unless nin = 1 (then only below the 128-tile kernel); never split-K with accumulate on an f16x3 kernel;
    a fused epilogue only on an unsplit plan; gemm_workspace_bytes covers the plan launch_gemm ends up on."""
    for mode, B, nin, nout, post in _grid():
        l = gp.linear_launches(mode, B, nin, nout, post, training=not post)
        for op in gp.OPS:
            g = l[op]
            M, N, K = {"fwd": (B, nout, nin), "dgrad": (B, nin, nout), "wgrad": (nout, nin, B)}[op]
            what = (mode, B, nin, nout, post, op, g.brief())
            assert g.kernel in gp.LABELS - {gp.REDUCE}, what
            assert (g.kernel != gp.MFMA) == (mode == "f16x3" and nin * nout >= 1 << 20), what
            if g.a_load == "strided" and g.b_load != "strided":
                assert nin == 1 and op == "wgrad" and g.kernel != gp.BIG, what
            assert not (g.kernel != gp.MFMA and g.nsplit > 1 and g.accumulate), what
            assert g.epilogue != "fused" or (g.nsplit == 1 and g.bias == "kernel"), what
            assert g.accumulate == (op == "wgrad") and (g.bias != "none") == (op == "fwd"), what
            assert (g.nsplit - 1) * g.klen < K <= g.nsplit * g.klen and g.klen % 32 == 0, what
            assert gp.gemm_workspace_bytes(M, N, K) >= gp.workspace_needed(g, M, N), what
            assert g.grid == (-(-N // (128 if g.kernel == gp.BIG else 64)), -(-M // (128 if g.kernel == gp.BIG else 64)), g.nsplit), what


# ---------------------------------------------------------------- the bound has teeth
TEETH = [("f32_split4_vec", "fwd"), ("f32_wgrad_split2", "wgrad"), ("f16x3_narrow_n_split66", "fwd"),      # K = 10500, the table's largest
         ("big_unsplit_scalar_mixed_stores", "fwd"),                                                         # K = 102, the smallest on an f16x3 kernel
         ("f16x3_split8", "fwd"), ("f16x3_split8", "dgrad")]


def _ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())


@pytest.mark.parametrize("name,op", TEETH, ids=[f"{n}-{o}" for n, o in TEETH])
def test_bound_accepts_correct_and_rejects_degraded_arithmetic(name, op):
    """On the case's data and plan.  Accepted (and under half the bound: the conv constants, measured to K = 1152, hold to K = 10500): fp32
    accumulated sequentially in K order per split, the splits added in order; on an f16x3 kernel also the three-product fp16 emulation.
    Rejected: f16x3 without one cross product, single-term fp16, the last split omitted, the bias added once per split, a tail column taken
    from its neighbour."""
    c = gp.BY_NAME[name]
    d = gp.inputs(c)
    ref, bound = gp.reference(c, op, d)
    plan = c.launches()[op]
    ratios = {}
    good = gp.emulate(c, op, d, "fp32")
    ratios["fp32"] = gp.check_bound(good, ref, bound, f"{name} {op}: fp32")
    if c.f16:
        ratios["f16x3"] = gp.check_bound(gp.emulate(c, op, d, "f16x3"), ref, bound, f"{name} {op}: f16x3")
        for kind in ("f16x3_without_x1w0", "fp16_single_term"):
            ratios[kind] = _ratio(gp.emulate(c, op, d, kind), ref, bound)
    if plan.nsplit > 1:
        ratios["last_split_omitted"] = _ratio(gp.emulate(c, op, d, "fp32", drop_last_split=True), ref, bound)
        if op == "fwd":
            ratios["bias_per_split"] = _ratio(gp.emulate(c, op, d, "fp32", bias_per_split=True), ref, bound)
    tail = good.copy()
    tail[:, -1] = tail[:, -2]
    ratios["tail_column_from_neighbour"] = _ratio(tail, ref, bound)
    print(f"{name} {op} ({plan.brief()}):", {k: round(v, 3) for k, v in ratios.items()})
    for kind, r in ratios.items():
        if kind in ("fp32", "f16x3"):
            assert r < 1.0, f"{name} {op}: the bound rejects the correct {kind} emulation ({r:.2f})"
            assert r < 0.5 or c.dims(op)[2] < 1152, f"{name} {op}: the correct {kind} emulation uses {r:.2f} of the bound - the conv constants (measured to K = 1152) do not carry over to this K"
        else:
            assert r > 1.0, f"{name} {op}: the bound accepts {kind} (max err / bound {r:.2f})"


EP_CASES = [c.name for c in gp.CASES if c.post]


def test_activation_constants_are_twice_the_measured_error():
    """C_ACT: float32 numpy activations against float64 on the pre-activations of the epilogue cases, relative to U * act_scale.  The
    measured ratios are printed (and recorded beside C_ACT); the constants are at least twice them."""
    worst = {}
    for name in EP_CASES:
        c = gp.BY_NAME[name]
        d = gp.inputs(c)
        y, _ = gp.reference(c, "fwd", d)
        out, p, _, _ = gp.epilogue64(c, d, y)
        p32 = p.astype(np.float32)
        o64 = gp.activation(c.act, p32.astype(np.float64))
        r = np.abs(gp.activation(c.act, p32).astype(np.float64) - o64) / (gp.U * np.maximum(gp.act_scale(c.act, p32.astype(np.float64), o64), 1e-300))
        worst[c.act] = max(worst.get(c.act, 0.0), float(r.max()))
    print("activation error / (U * scale):", {k: round(v, 3) for k, v in sorted(worst.items())})
    for act, r in worst.items():
        assert gp.C_ACT[act] >= 2 * r, (act, r, gp.C_ACT[act])


@pytest.mark.parametrize("name", ["ep_f32_bn_elu", "ep_bf16x6_bn_leakyrelu", "ep_f32_bn_tanh", "ep_f32_sigmoid", "ep_f32_bn_alone", "ep_f16x3_bn_relu"])
def test_epilogue_bound_accepts_the_fp32_epilogue_and_rejects_a_wrong_one(name):
    """The propagated bound accepts the fp32 emulation of gemm_store_block's epilogue on the emulated GEMM output, and rejects gamma applied
    before invstd with beta dropped (cases with BatchNorm), and a tail column taken from its neighbour."""
    c = gp.BY_NAME[name]
    d = gp.inputs(c)
    ref, bound = gp.reference_epilogue(c, d)
    y = gp.emulate(c, "fwd", d, "f16x3" if c.f16 else "fp32")
    good = gp.emulate_epilogue(c, d, y)
    ratios = {"fp32_epilogue": gp.check_bound(good, ref, bound, name)}
    if c.bn:
        ratios["gamma_first_beta_dropped"] = _ratio(gp.emulate_epilogue(c, d, y, wrong=True), ref, bound)
    tail = good.copy()
    tail[:, -1] = tail[:, -2]
    ratios["tail_column_from_neighbour"] = _ratio(tail, ref, bound)
    print(name, {k: round(v, 3) for k, v in ratios.items()})
    assert ratios.pop("fp32_epilogue") < 0.5
    for kind, r in ratios.items():
        assert r > 1.0, f"{name}: the bound accepts {kind} (max err / bound {r:.2f})"
