"""CPU checks of tests/conv_paths.py: the case table reaches every leaf of the restated convolution dispatch at the shapes where kernels go
wrong, and the per-element float64 bound accepts correct emulations of the three arithmetic modes while rejecting subtly degraded ones."""
import numpy as np
import pytest

import conv_paths as cp


def test_case_table_reaches_every_leaf():
    """Each case's expected kernels are what the mirror predicts for it; together they reach every leaf; the mirror names nothing else."""
    reached = set()
    for c in cp.CASES:
        assert c.mirror() == c.leaves(), (c.name, sorted(c.mirror()), sorted(c.leaves()))
        reached |= c.leaves()
    assert len(cp.BY_NAME) == len(cp.CASES) + len(cp.NET_CASES), "case names are unique"
    assert reached == set(cp.LEAVES), f"leaves no case reaches: {sorted(set(cp.LEAVES) - reached)}; labels outside LEAVES: {sorted(reached - cp.LEAVES)}"
    net = set()
    for c in cp.NET_CASES:
        assert c.mirror() == c.leaves(), (c.name, sorted(c.mirror()), sorted(c.leaves()))
        net |= c.leaves()
    assert net == set(cp.NET_LEAVES), f"net leaves no case reaches: {sorted(set(cp.NET_LEAVES) - net)}; outside NET_LEAVES: {sorted(net - cp.NET_LEAVES)}"


def test_mirror_names_only_leaves():
    """Every label the mirror produces over a grid of shapes, modes and knobs is an element of LEAVES."""
    seen = set()
    for mode in cp.MODES:
        for B in (1, 3, 9, 64, 257):
            for Cin, Cout in ((1, 64), (3, 3), (5, 1), (8, 4), (16, 20), (24, 64), (40, 100), (128, 256)):
                for H, W in ((4, 4), (8, 8), (7, 13), (16, 16), (12, 16), (17, 33), (32, 32), (22, 36), (64, 64), (30, 64)):
                    for up in (False, True):
                        if up and (H % 2 or W % 2):
                            continue
                        for s8 in (1, 128):
                            seen |= cp.forward_leaves(mode, B, Cin, Cout, H, W, up, s8)
                    seen |= cp.backward_data_leaves(mode, B, Cin, Cout, H, W)
                    seen |= cp.backward_weight_leaves(mode, B, Cin, Cout, H, W)
                    for k in (3, 5):
                        seen_net = cp.net_stage_leaves(mode, B, Cin, Cout, H, W, k)
                        assert seen_net <= cp.NET_LEAVES, sorted(seen_net - cp.NET_LEAVES)
    assert seen <= cp.LEAVES, sorted(seen - cp.LEAVES)


def test_cases_sit_where_kernels_go_wrong():
    """Odd widths on every split leaf that admits them, ragged last tiles, Cin off the chunk, Cout off the 32-channel block, the smallest
    planes, persistent grids with more tiles than resident workgroups."""
    split = [c for c in cp.CASES if c.expect.startswith("conv3x3_split") and c.op != "wgrad"]
    for leaf in {c.expect for c in cp.CASES if c.op != "wgrad"}:
        cs = [c for c in cp.CASES if c.expect == leaf]
        cin = [c.Cout if c.op == "dgrad" else c.Cin for c in cs]          # the launch's input and output channels
        cout = [c.Cin if c.op == "dgrad" else c.Cout for c in cs]
        if leaf.startswith("conv3x3_split") or leaf.startswith("conv3x3_up2"):
            stacked = leaf.endswith(", 4>") or leaf.startswith("conv3x3_split_wide_kernel<16") or leaf.startswith("conv3x3_up2_f16x3")
            TW = int(leaf.split("<")[1].split(",")[0])
            if not stacked:                                              # (stacked tiles hold whole 8x8 / 16x16 planes)
                assert leaf.startswith("conv3x3_up2") or any(c.W % 2 for c in cs if not c.up), f"{leaf}: an odd width"
                assert any((c.W // (2 if c.up else 1)) % TW for c in cs), f"{leaf}: a ragged last tile in x"
            assert any(v % 16 for v in cin), f"{leaf}: Cin off the 16-channel chunk"
            assert any(v % 32 for v in cout), f"{leaf}: Cout off the 32-channel block"
        elif leaf.startswith("conv3x3_mfma"):
            TW = int(leaf.split(", ")[1])
            assert any(v % 8 for v in cin), f"{leaf}: Cin off the 8-channel chunk"
            assert any(v % 32 for v in cout) or leaf.startswith("conv3x3_mfma_kernel<1"), f"{leaf}: Cout off the block"
            assert any(c.W % TW for c in cs), f"{leaf}: a ragged last tile in x"
        elif "fewout" in leaf:
            assert any(v % 8 for v in cin) or leaf.endswith("64>"), f"{leaf}: Cin off the 8-channel chunk"
    for N in (2, 3):
        for fam in ("conv3x3_split_kernel<8, 1", "conv3x3_split_kernel<16, 2", "conv3x3_split_kernel<32, 2"):
            assert any(c.up and c.expect.startswith(f"{fam}, {N}") for c in split), f"{fam}, {N}>: up-sampled input"
        assert any(c.expect.startswith("conv3x3_split_wide_kernel<16") and cp.split_wide_tiles(N, c.B, c.Cout, c.H, c.W) > cp.RESIDENT_WIDE[N]
                   for c in split if ("3" if N == 3 else "2") == c.expect.split(", ")[2]), f"split_wide<16> NTERM {N}: persistent grid"
        assert any(c.expect.startswith("conv3x3_split_wide_kernel<32") and cp.split_wide_tiles(N, c.B, c.Cout, c.H, c.W) > cp.RESIDENT_WIDE[N]
                   for c in split if ("3" if N == 3 else "2") == c.expect.split(", ")[2]), f"split_wide<32> NTERM {N}: persistent grid"
    assert any(c.Cin % 16 for c in split) and any(c.Cin % 8 for c in cp.CASES if "mfma" in c.expect), "Cin off the chunk"
    assert any(c.B % 4 for c in split if c.expect.endswith(", 4>")), "a half-empty stacked 8x8 tile"
    assert any(c.B % 8 for c in cp.CASES if c.expect.startswith("conv3x3_up2_f16x3_kernel<8, 8")), "a half-empty 8-image up-sampling tile"
    fo = [c for c in cp.CASES if "fewout" in c.expect]
    assert any(c.W == 16 and c.H == 8 for c in fo) and any(c.W == 16 and c.H % 8 for c in fo), "the smallest few-output planes"
    assert any(c.H % 16 for c in fo if ", 64>" in c.expect) and any(c.W % 32 and c.H % 32 for c in fo if c.expect.endswith("1, 32>"))
    assert {m for c in cp.CASES for m in [c.mode]} == set(cp.MODES)
    assert any(c.W % 2 for c in cp.CASES if c.op == "wgrad") and any(c.H % 2 for c in cp.CASES if "wgrad_split_kernel" in c.expect)


# ---------------------------------------------------------------- the bound has teeth
TEETH_CASES = ["fwd_bf16x6_split8_odd", "fwd_f16x3_split16_mt1_odd", "fwd_bf16x6_split32_mt2_odd", "fwd_f16x3_split8_stack4_wide",
               "fwd_bf16x6_wide32_odd_persistent"]


@pytest.mark.parametrize("name", TEETH_CASES)
def test_bound_accepts_correct_and_rejects_degraded_arithmetic(name):
    """On the case's shape and data: fp32 torch and correct bf16x6 / f16x3 emulations stay inside the bound of their mode; the bf16 split
    without its order-2 products, f16x3 without one cross product and single-term fp16 do not."""
    c = cp.BY_NAME[name]
    x, w, b, dy, gw0 = cp.inputs(c)
    bounds = {}
    for mode in ("f32", "bf16x6", "f16x3"):
        ref, bounds[mode] = cp.reference(cp.Case(c.name, "fwd", mode, c.B, c.Cin, c.Cout, c.H, c.W, c.expect), x, w, b, dy, gw0)
    ratios = {}
    for kind, mode in (("fp32", "f32"), ("bf16x6", "bf16x6"), ("f16x3", "f16x3")):
        y = cp.emulate_forward(kind, x, w, b)
        ratios[kind] = cp.check_bound(y, ref, bounds[mode], f"{name}: {kind}")
    for kind, mode in (("bf16x6_without_order2", "bf16x6"), ("f16x3_without_x1w0", "f16x3"), ("fp16_single_term", "f16x3")):
        y = cp.emulate_forward(kind, x, w, b)
        err = np.abs(y.astype(np.float64) - ref)
        ratios[kind] = float((err / bounds[mode]).max())
        assert ratios[kind] > 1.0, f"{name}: the {mode} bound accepts {kind} (max err / bound {ratios[kind]:.2f})"
    print(name, {k: round(v, 2) for k, v in ratios.items()})
