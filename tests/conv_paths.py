"""The 3x3 convolution dispatch of the stand-alone entry points, restated; a case table that reaches every leaf; a float64 reference and a
per-element error bound that separates a correct fp32-class kernel from a subtly wrong one.

Used by tests/test_conv_paths_host.py (CPU: the table reaches every leaf, the mirror names no label outside LEAVES, the bound accepts correct
emulations of the three arithmetic modes and rejects degraded ones) and tests/test_gpu_conv_paths.py (every case against the bound, and its
kernel_times() labels against the mirror).

Scope: what gr_conv3_forward_dev, gr_conv3_backward_data_dev and gr_conv3_backward_weight_dev (ops.hip) can launch - launch_conv3x3 (fp32
MFMA and few-output VALU kernels), launch_conv3x3_split_n (bf16x6 / f16x3), launch_conv3x3_up2_f16x3 and launch_conv3x3_wgrad.  The kernels
only a net launches (conv3x3_fewin*, the 5x5 kernels of conv.hip / convk.hip) are restated further down as one-stage nets; the operand-ready
(P16) kernels, which need a producer stage in front of them, have a module of their own: tests/p16_paths.py."""
import dataclasses
import math
import zlib

import numpy as np

# ---------------------------------------------------------------- the dispatch, restated (gan-reverser_amd/csrc)
MODES = {"f32": 0, "bf16x6": 1, "f16x3": 2}
RESIDENT_WIDE = {2: 256, 3: 512}      # conv.hip launch_conv_split_wide_db: persistent workgroups (f16x3 double-buffered: one per CU)
WGRAD_REDUCE = "conv3x3_wgrad_reduce8_kernel"
WGRAD_SMALL_REDUCE = "conv3x3_wgrad_small_reduce_kernel"


def round_up(v, m):
    return (v + m - 1) // m * m


def conv_up2_supported(Cin, Cout, H, W):
    """conv.hip conv_up2_supported (H, W: the output plane)"""
    Hs, Ws = H // 2, W // 2
    if H % 2 or W % 4 or Cout <= 4:
        return False
    return (Hs == 8 and Ws == 8) or (Hs == 16 and Ws == 16) or Ws >= 17


def up2_leaf(W):
    """launch_conv3x3_up2_f16x3 (conv.hip): 8-wide source planes <8, 8>, 16-wide <16, 2>, else up2q<32, 1>; DB where two LDS images fit
    (launch_conv_up2_t's FITS)"""
    def fits(TW, NI):
        IH = 512 // (NI * TW)
        PSL = round_up(NI * (IH + 2) * (TW + 2), 16)
        return 2 * 16 * (2 * 2 * PSL + 2 * 2 * 8 * 2 * 32) + 5 * 32 * 4 <= 160 * 1024
    Ws = W // 2
    if Ws == 8:
        return f"conv3x3_up2_f16x3_kernel<8, 8, {str(fits(8, 8)).lower()}>"
    if Ws == 16:
        return f"conv3x3_up2_f16x3_kernel<16, 2, {str(fits(16, 2)).lower()}>"
    return "conv3x3_up2q_f16x3_kernel<32, 1>"


def mfma_leaf(B, Cout, H, W, w_native, up):
    """launch_conv3x3 (conv.hip): the few-output VALU kernel when the caller passes native weights, else the fp32 MFMA kernel"""
    if w_native and Cout <= 4 and not up and W % 4 == 0 and W >= 16:
        ks4 = H % 16 == 0 and ((W + 31) // 32) * ((H + 31) // 32) < 4
        wide64 = not ks4 and W % 64 == 0
        return f"conv3x3_fewout_kernel<{Cout}, " + ("4, 32>" if ks4 else ("1, 64>" if wide64 else "1, 32>"))
    if round_up(Cout, 32) % 64 != 0:
        MT, NG = 1, 2
    elif H * W >= 512 and W >= 32:
        return "conv3x3_mfma_kernel<2, 32, 4>"
    else:
        MT, NG = 2, 2
    TW = 8 if W <= 8 else (16 if W <= 16 else 32)
    return f"conv3x3_mfma_kernel<{MT}, {TW}, {2 if TW == 8 else NG}>"        # launch_conv_mt: 8-wide tiles always NG = 2


def split_leaf(N, B, Cout, H, W, up, stack8):
    """launch_conv3x3_split_n<NTERM> (conv.hip); stack8 = g_stack8_min_wgs"""
    cp = round_up(Cout, 32)
    wide = cp % 64 == 0
    st_tiles, cp32 = (B + 3) // 4, cp // 32
    if W == 8 and H == 8 and not up and wide and st_tiles * (cp32 // 2) >= stack8:
        return f"conv3x3_split_kernel<8, 2, {N}, 4>"
    if W == 8 and H == 8 and not up and st_tiles * cp32 >= stack8:
        return f"conv3x3_split_kernel<8, 1, {N}, 4>"
    db = "true" if N == 2 else "false"
    if W <= 8:
        return f"conv3x3_split_kernel<8, 1, {N}>"
    if W <= 16:
        if wide and H == 16 and W == 16 and ((B + 1) // 2) * (cp // 64) >= 256:
            return f"conv3x3_split_wide_kernel<16, 2, {N}, {db}>"
        return f"conv3x3_split_kernel<16, {2 if wide else 1}, {N}>"
    if wide and H * W >= 512 and B * ((H * W + 511) // 512) * (cp // 64) >= 256:
        return f"conv3x3_split_wide_kernel<32, 1, {N}, {db}>"
    return f"conv3x3_split_kernel<32, {2 if wide else 1}, {N}>"


def split_wide_tiles(N, B, Cout, H, W):
    """Tiles of a split_wide launch (launch_conv_split_wide_db): 16x16 planes two to a tile, else 32 x 16 tiles"""
    otiles = round_up(Cout, 32) // 64
    if H == 16 and W == 16:
        return (B + 1) // 2 * otiles
    return B * ((W + 31) // 32) * ((H + 15) // 16) * otiles


def forward_leaves(mode, B, Cin, Cout, H, W, up, stack8=128):
    """gr_conv3_forward_dev (ops.hip): H, W = the output plane (the input is H/2 x W/2 when up)"""
    m = MODES[mode]
    if m == 2 and up and conv_up2_supported(Cin, Cout, H, W):
        return {up2_leaf(W)}
    if m >= 1 and Cout > 4:
        return {split_leaf(2 if m == 2 else 3, B, Cout, H, W, up, stack8)}
    return {mfma_leaf(B, Cout, H, W, True, up)}


def backward_data_leaves(mode, B, Cin, Cout, H, W, stack8=128):
    """gr_conv3_backward_data_dev (ops.hip): the forward kernels with Cin and Cout exchanged, no native weights (no few-output kernel)"""
    m = MODES[mode]
    if m >= 1 and Cin > 4:
        return {split_leaf(2 if m == 2 else 3, B, Cin, H, W, False, stack8)}
    return {mfma_leaf(B, Cin, H, W, False, False)}


def wgrad_geometry(mode, B, Cin, Cout, H, W):
    """conv.hip wgrad_geometry: (TW, split, small, vec, tiles_x, nsplit)"""
    m = MODES[mode]
    TW = 8 if W <= 8 else (16 if W <= 16 else 32)
    vec = W >= 16 and W % 4 == 0
    small = Cin <= 3 and W >= 16 and W % 4 == 0
    split = m >= 1 and Cin > 3 and W >= 16 and W % 8 == 0
    TR = (32 if split else 64) // TW
    tiles_x, tiles_y = (W + TW - 1) // TW, (H + TR - 1) // TR
    tiles_total = B * tiles_x * tiles_y
    n_ob, n_cb = round_up(Cout, 64) // 64, round_up(Cin, 64) // 64
    want = (256 if vec else 512) // (n_ob * n_cb)
    if small:
        want = 1024 // n_ob
    elif split:
        want = (512 if (TW == 32 and B * H * tiles_x >= 16384) else 256) // (n_ob * n_cb)
    nsplit = min(max(want, 1), tiles_total)
    return TW, split, small, vec, tiles_x, nsplit


def wgrad_rows_per_segment(B, H, TW, tiles_x, nsplit):
    """launch_conv3x3_wgrad's rps (0: the per-tile split kernel)"""
    TRr = 32 // TW
    if H % TRr:
        return 0
    for cand in range(H, TRr - 1, -1):
        if H % cand == 0 and cand % TRr == 0:
            nsegs = B * (H // cand) * tiles_x
            if nsegs >= nsplit and (nsegs % nsplit == 0 or nsegs >= 4 * nsplit or cand == TRr):
                return cand
    return 0


def backward_weight_leaves(mode, B, Cin, Cout, H, W):
    """gr_conv3_backward_weight_dev -> launch_conv3x3_wgrad (conv.hip)"""
    TW, split, small, vec, tiles_x, nsplit = wgrad_geometry(mode, B, Cin, Cout, H, W)
    N = 2 if MODES[mode] == 2 else 3
    if split:
        rps = wgrad_rows_per_segment(B, H, TW, tiles_x, nsplit)
        k = f"conv3x3_wgrad_split_roll_kernel<{TW}, {N}>" if rps else f"conv3x3_wgrad_split_kernel<{TW}, 2, {N}>"
        return {k, WGRAD_REDUCE}
    if small:
        return {f"conv3x3_wgrad_small_kernel<{TW}>", WGRAD_SMALL_REDUCE}
    if vec:
        return {f"conv3x3_wgrad_vec_kernel<{TW}>", WGRAD_REDUCE}
    return {f"conv3x3_wgrad_kernel<{TW}>", WGRAD_REDUCE}


def all_mirror_leaves():
    """Every label the restated dispatch can produce, by enumeration over the template choices it makes"""
    out = set()
    for MT, TW in [(1, 8), (1, 16), (1, 32), (2, 8), (2, 16), (2, 32)]:
        out.add(f"conv3x3_mfma_kernel<{MT}, {TW}, 2>")
    out.add("conv3x3_mfma_kernel<2, 32, 4>")
    for co in range(1, 5):
        out |= {f"conv3x3_fewout_kernel<{co}, 4, 32>", f"conv3x3_fewout_kernel<{co}, 1, 64>", f"conv3x3_fewout_kernel<{co}, 1, 32>"}
    for N in (2, 3):
        db = "true" if N == 2 else "false"
        out |= {f"conv3x3_split_kernel<8, 1, {N}>", f"conv3x3_split_kernel<8, 1, {N}, 4>", f"conv3x3_split_kernel<8, 2, {N}, 4>",
                f"conv3x3_split_kernel<16, 1, {N}>", f"conv3x3_split_kernel<16, 2, {N}>", f"conv3x3_split_kernel<32, 1, {N}>",
                f"conv3x3_split_kernel<32, 2, {N}>", f"conv3x3_split_wide_kernel<16, 2, {N}, {db}>", f"conv3x3_split_wide_kernel<32, 1, {N}, {db}>"}
        for TW in (16, 32):       # (the per-tile split kernel: only when rps = 0, i.e. on 16-wide tiles; the enumeration asks the mirror)
            out.add(f"conv3x3_wgrad_split_roll_kernel<{TW}, {N}>")
    for W in (16, 32, 36):
        out.add(up2_leaf(W))
    for TW in (8, 16, 32):
        out.add(f"conv3x3_wgrad_kernel<{TW}>")
    for TW in (16, 32):
        out |= {f"conv3x3_wgrad_vec_kernel<{TW}>", f"conv3x3_wgrad_small_kernel<{TW}>"}
    out |= {WGRAD_REDUCE, WGRAD_SMALL_REDUCE}
    # the per-tile split wgrad kernel, enumerated through the mirror itself: rps = 0 needs an odd H, which only 16-wide tiles notice
    for mode in ("bf16x6", "f16x3"):
        for W in (16, 24, 32, 40, 64):
            for H in (1, 2, 3, 7, 8, 9, 16, 31, 32):
                for B in (1, 2, 64, 512):
                    out |= backward_weight_leaves(mode, B, 16, 64, H, W)
    return out


LEAVES = frozenset(all_mirror_leaves())


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    op: str            # "fwd", "dgrad" or "wgrad"
    mode: str
    B: int
    Cin: int
    Cout: int
    H: int             # the output plane (the layer's input is H/2 x W/2 when up)
    W: int
    expect: str        # the convolution kernel the case is about (wgrad: + its reduce kernel, added by leaves())
    up: bool = False
    stack8: int = 128  # gr_set_tuning("stack8_min_wgs") for the case (the library default: 128)

    def leaves(self):
        k = {self.expect}
        if self.op == "wgrad":
            k.add(WGRAD_SMALL_REDUCE if "small" in self.expect else WGRAD_REDUCE)
        return k

    def mirror(self):
        if self.op == "fwd":
            return forward_leaves(self.mode, self.B, self.Cin, self.Cout, self.H, self.W, self.up, self.stack8)
        if self.op == "dgrad":
            return backward_data_leaves(self.mode, self.B, self.Cin, self.Cout, self.H, self.W, self.stack8)
        return backward_weight_leaves(self.mode, self.B, self.Cin, self.Cout, self.H, self.W)


def _split_cases(mode, N):
    db = "true" if N == 2 else "false"
    m = mode
    wide16_cout = 100 if N == 2 else 228     # 129 two-image tiles x 2 (x 4) channel blocks: more tiles than the 256 (512) resident workgroups
    return [
        Case(f"fwd_{m}_split8_odd", "fwd", m, 3, 20, 40, 5, 7, f"conv3x3_split_kernel<8, 1, {N}>"),
        Case(f"fwd_{m}_split8_up", "fwd", m, 2, 24, 36, 8, 8, f"conv3x3_split_kernel<8, 1, {N}>", up=True),
        Case(f"fwd_{m}_split8_stack4_ragged", "fwd", m, 9, 20, 20, 8, 8, f"conv3x3_split_kernel<8, 1, {N}, 4>", stack8=1),
        Case(f"fwd_{m}_split8_stack4_wide", "fwd", m, 6, 40, 100, 8, 8, f"conv3x3_split_kernel<8, 2, {N}, 4>", stack8=1),
        Case(f"fwd_{m}_split16_mt1_odd", "fwd", m, 2, 24, 30, 19, 13, f"conv3x3_split_kernel<16, 1, {N}>"),
        Case(f"fwd_{m}_split16_mt2_odd", "fwd", m, 2, 17, 40, 16, 9, f"conv3x3_split_kernel<16, 2, {N}>"),
        Case(f"fwd_{m}_split16_up", "fwd", m, 2, 16, 64, 12, 16, f"conv3x3_split_kernel<16, 2, {N}>", up=True),
        Case(f"fwd_{m}_split32_mt1_odd", "fwd", m, 2, 18, 20, 7, 17, f"conv3x3_split_kernel<32, 1, {N}>"),
        Case(f"fwd_{m}_split32_mt2_odd", "fwd", m, 2, 40, 120, 15, 33, f"conv3x3_split_kernel<32, 2, {N}>"),
        Case(f"fwd_{m}_split32_up", "fwd", m, 2, 24, 64, 20, 34, f"conv3x3_split_kernel<32, 2, {N}>", up=True),
        Case(f"fwd_{m}_wide16_persistent", "fwd", m, 257, 8, wide16_cout, 16, 16, f"conv3x3_split_wide_kernel<16, 2, {N}, {db}>"),
        Case(f"fwd_{m}_wide32_odd_persistent", "fwd", m, 65, 8, 100, 17, 33, f"conv3x3_split_wide_kernel<32, 1, {N}, {db}>"),
    ]


CASES = [
    # fp32 MFMA (f32 mode; and every mode's data gradient with Cin <= 4): MT 1 / 2 x TW 8 / 16 / 32, and the 512-pixel tile
    Case("fwd_f32_mfma_mt1_tw8", "fwd", "f32", 3, 5, 20, 5, 7, "conv3x3_mfma_kernel<1, 8, 2>"),
    Case("fwd_f32_mfma_mt1_tw16", "fwd", "f32", 2, 12, 70, 11, 13, "conv3x3_mfma_kernel<1, 16, 2>"),
    Case("fwd_f32_mfma_mt1_tw32", "fwd", "f32", 2, 9, 30, 9, 33, "conv3x3_mfma_kernel<1, 32, 2>"),
    Case("fwd_f32_mfma_mt2_tw8", "fwd", "f32", 2, 3, 50, 7, 6, "conv3x3_mfma_kernel<2, 8, 2>"),
    Case("fwd_f32_mfma_mt2_tw16", "fwd", "f32", 2, 17, 100, 17, 15, "conv3x3_mfma_kernel<2, 16, 2>"),
    Case("fwd_f32_mfma_mt2_tw32", "fwd", "f32", 2, 11, 50, 12, 40, "conv3x3_mfma_kernel<2, 32, 2>"),
    Case("fwd_f32_mfma_512px", "fwd", "f32", 2, 10, 120, 20, 33, "conv3x3_mfma_kernel<2, 32, 4>"),
    Case("fwd_bf16x6_up_narrow_out_mfma", "fwd", "bf16x6", 2, 16, 3, 10, 12, "conv3x3_mfma_kernel<1, 16, 2>", up=True),
    Case("dgrad_f32_mfma", "dgrad", "f32", 2, 40, 24, 16, 16, "conv3x3_mfma_kernel<2, 16, 2>"),
    Case("dgrad_f16x3_cin3_mfma", "dgrad", "f16x3", 2, 3, 32, 16, 16, "conv3x3_mfma_kernel<1, 16, 2>"),
    # few output channels (every mode): KS = 4 on small planes, 64-wide tiles, generic 32-row tiles; CO 1 .. 4
    Case("fwd_f16x3_fewout1_ks4", "fwd", "f16x3", 2, 124, 1, 16, 16, "conv3x3_fewout_kernel<1, 4, 32>"),
    Case("fwd_bf16x6_fewout2_ks4", "fwd", "bf16x6", 3, 21, 2, 32, 48, "conv3x3_fewout_kernel<2, 4, 32>"),
    Case("fwd_f32_fewout3_ks4_smallest", "fwd", "f32", 1, 7, 3, 16, 16, "conv3x3_fewout_kernel<3, 4, 32>"),
    Case("fwd_f32_fewout3_generic_h8", "fwd", "f32", 1, 7, 3, 8, 16, "conv3x3_fewout_kernel<3, 1, 32>"),     # small, but 8 rows: not KS = 4
    Case("fwd_f32_fewout2_w64_h24", "fwd", "f32", 1, 8, 2, 24, 64, "conv3x3_fewout_kernel<2, 1, 64>"),
    Case("fwd_f32_fewout4_ks4", "fwd", "f32", 2, 9, 4, 48, 16, "conv3x3_fewout_kernel<4, 4, 32>"),
    Case("fwd_f32_fewout1_w64_ragged_rows", "fwd", "f32", 2, 16, 1, 30, 64, "conv3x3_fewout_kernel<1, 1, 64>"),
    Case("fwd_f16x3_fewout2_w64", "fwd", "f16x3", 1, 33, 2, 64, 128, "conv3x3_fewout_kernel<2, 1, 64>"),
    Case("fwd_bf16x6_fewout3_w64", "fwd", "bf16x6", 2, 128, 3, 17, 64, "conv3x3_fewout_kernel<3, 1, 64>"),
    Case("fwd_f32_fewout4_w64", "fwd", "f32", 1, 5, 4, 64, 64, "conv3x3_fewout_kernel<4, 1, 64>"),
    Case("fwd_f32_fewout1_generic_smallest", "fwd", "f32", 3, 10, 1, 12, 16, "conv3x3_fewout_kernel<1, 1, 32>"),
    Case("fwd_f16x3_fewout2_generic", "fwd", "f16x3", 2, 27, 2, 40, 40, "conv3x3_fewout_kernel<2, 1, 32>"),
    Case("fwd_bf16x6_fewout3_generic", "fwd", "bf16x6", 2, 17, 3, 33, 36, "conv3x3_fewout_kernel<3, 1, 32>"),
    Case("fwd_f32_fewout4_generic_many_tiles", "fwd", "f32", 1, 13, 4, 96, 100, "conv3x3_fewout_kernel<4, 1, 32>"),
    # split kernels (bf16x6: three terms, f16x3: two), forward and data gradient
    *_split_cases("bf16x6", 3),
    *_split_cases("f16x3", 2),
    Case("dgrad_bf16x6_split8_odd", "dgrad", "bf16x6", 2, 40, 24, 13, 7, "conv3x3_split_kernel<8, 1, 3>"),
    Case("dgrad_f16x3_split16", "dgrad", "f16x3", 3, 64, 20, 16, 16, "conv3x3_split_kernel<16, 2, 2>"),
    # up-sampling f16x3 kernels (four 2x2 convolutions of the source plane): ragged 8-image tiles, odd batch, ragged 32-wide source tiles
    Case("fwd_f16x3_up2_8x8_ragged", "fwd", "f16x3", 9, 20, 40, 16, 16, "conv3x3_up2_f16x3_kernel<8, 8, false>", up=True),
    Case("fwd_f16x3_up2_16x16", "fwd", "f16x3", 3, 20, 36, 32, 32, "conv3x3_up2_f16x3_kernel<16, 2, true>", up=True),
    Case("fwd_f16x3_up2q_ragged", "fwd", "f16x3", 2, 24, 72, 22, 36, "conv3x3_up2q_f16x3_kernel<32, 1>", up=True),
    # weight gradient: rolling-window and per-tile split kernels, small-Cin, vector and plain fp32 kernels
    Case("wgrad_bf16x6_roll16", "wgrad", "bf16x6", 2, 24, 40, 14, 16, "conv3x3_wgrad_split_roll_kernel<16, 3>"),
    Case("wgrad_f16x3_roll16", "wgrad", "f16x3", 3, 8, 100, 16, 16, "conv3x3_wgrad_split_roll_kernel<16, 2>"),
    Case("wgrad_f16x3_roll32", "wgrad", "f16x3", 2, 20, 24, 9, 24, "conv3x3_wgrad_split_roll_kernel<32, 2>"),
    Case("wgrad_bf16x6_roll32", "wgrad", "bf16x6", 2, 16, 70, 7, 40, "conv3x3_wgrad_split_roll_kernel<32, 3>"),
    Case("wgrad_bf16x6_split16_odd_rows", "wgrad", "bf16x6", 2, 12, 36, 15, 16, "conv3x3_wgrad_split_kernel<16, 2, 3>"),
    Case("wgrad_f16x3_split16_odd_rows", "wgrad", "f16x3", 1, 40, 8, 9, 16, "conv3x3_wgrad_split_kernel<16, 2, 2>"),
    Case("wgrad_f16x3_small16", "wgrad", "f16x3", 3, 1, 64, 16, 16, "conv3x3_wgrad_small_kernel<16>"),
    Case("wgrad_bf16x6_small32", "wgrad", "bf16x6", 2, 3, 40, 12, 20, "conv3x3_wgrad_small_kernel<32>"),
    Case("wgrad_f32_vec16", "wgrad", "f32", 2, 24, 40, 10, 16, "conv3x3_wgrad_vec_kernel<16>"),
    Case("wgrad_f16x3_vec32", "wgrad", "f16x3", 2, 12, 36, 9, 20, "conv3x3_wgrad_vec_kernel<32>"),
    Case("wgrad_f16x3_plain8", "wgrad", "f16x3", 3, 20, 40, 8, 8, "conv3x3_wgrad_kernel<8>"),
    Case("wgrad_bf16x6_plain16_odd", "wgrad", "bf16x6", 2, 24, 33, 11, 13, "conv3x3_wgrad_kernel<16>"),
    Case("wgrad_f32_plain32_odd", "wgrad", "f32", 2, 8, 64, 7, 17, "conv3x3_wgrad_kernel<32>"),
]
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- the kernels only a net launches: one-stage nets (net.hip fwd_conv3 /
# fwd_convk / bwd_convk), the stage's input = the net input, its output = the raw convolution
CONVK_TILE, CONVK_SLICED_BELOW_WGS = 16, 1024      # convk.hip KC_TILE, convk_direct's SLICED_BELOW_WGS


def conv5x5_split_supported(Cin, Cout, H, W):
    """conv.hip conv5x5_split_supported"""
    return Cin >= 16 and Cin % 8 == 0 and W >= 8 and H >= 4


def conv5x5_leaf(W):
    """launch_conv5x5_split (conv.hip)"""
    return f"conv5x5_split_kernel<{8 if W <= 8 else (16 if W <= 16 else 32)}, 1, 2>"


def convk_direct_leaf(B, cout_eff, H, W, bwd):
    """convk.hip convk_direct: the sliced kernel below 1024 workgroups"""
    wgs = ((W + CONVK_TILE - 1) // CONVK_TILE) * ((H + CONVK_TILE - 1) // CONVK_TILE) * (round_up(cout_eff, 32) // 16) * B
    name = "convk_direct_sliced_kernel<5, 16, 4>" if wgs < CONVK_SLICED_BELOW_WGS else "convk_direct_kernel<5, 16, 1>"
    return name + ("(dgrad)" if bwd else "")


def net_stage_leaves(mode, B, Cin, Cout, H, W, ksz):
    """The net-only kernels a one-stage net's forward + backward (data and weight gradient) launches.  3x3: the few-input kernel
    (fwd_conv3, conv_fewin_applies); its data and weight gradients are stand-alone leaves (LEAVES), not restated for nets.  5x5: fwd_convk and
    bwd_convk (convk_split: f16x3 and a supported shape)."""
    if ksz == 3:
        return {f"conv3x3_fewin_kernel<{Cin}>"} if Cin <= 3 and W % 4 == 0 and W >= 4 else set()
    split = mode == "f16x3" and conv5x5_split_supported(Cin, Cout, H, W)
    out = {"convk_wgrad_kernel", "convk_wgrad_reduce_kernel"}
    out.add(conv5x5_leaf(W) if split else convk_direct_leaf(B, Cout, H, W, False))
    out.add(conv5x5_leaf(W) if split and conv5x5_split_supported(Cout, Cin, H, W) else convk_direct_leaf(B, Cin, H, W, True))
    return out


NET_LEAVES = frozenset({f"conv3x3_fewin_kernel<{c}>" for c in (1, 2, 3)} | {conv5x5_leaf(W) for W in (8, 16, 32)}
                       | {convk_direct_leaf(B, 32, 16, 16, bwd) for B in (1, 1024) for bwd in (False, True)}
                       | {"convk_wgrad_kernel", "convk_wgrad_reduce_kernel"})


@dataclasses.dataclass(frozen=True)
class NetCase:
    name: str
    mode: str
    B: int
    Cin: int
    Cout: int
    H: int
    W: int
    ksz: int
    expect: tuple      # the net-only kernels forward + backward launch
    op: str = "net"
    up: bool = False

    def leaves(self):
        return set(self.expect)

    def mirror(self):
        return net_stage_leaves(self.mode, self.B, self.Cin, self.Cout, self.H, self.W, self.ksz)


_KW = ("convk_wgrad_kernel", "convk_wgrad_reduce_kernel")
NET_CASES = [
    # few input channels: the smallest width (4), ragged 32-pixel tiles, Cout off the 8-channel slices
    NetCase("net_f32_fewin1_w4", "f32", 2, 1, 20, 13, 4, 3, ("conv3x3_fewin_kernel<1>",)),
    NetCase("net_bf16x6_fewin2", "bf16x6", 3, 2, 64, 33, 36, 3, ("conv3x3_fewin_kernel<2>",)),
    NetCase("net_f16x3_fewin3", "f16x3", 2, 3, 40, 17, 20, 3, ("conv3x3_fewin_kernel<3>",)),
    # 5x5 on the f16x3 split kernel (forward and data gradient): the smallest width (8), odd widths, ragged tiles, Cin off 16
    NetCase("net_f16x3_5x5_split8", "f16x3", 2, 16, 24, 6, 8, 5, ("conv5x5_split_kernel<8, 1, 2>",) + _KW),
    NetCase("net_f16x3_5x5_split16_odd", "f16x3", 2, 24, 40, 9, 13, 5, ("conv5x5_split_kernel<16, 1, 2>",) + _KW),
    NetCase("net_f16x3_5x5_split32_odd", "f16x3", 2, 32, 16, 5, 33, 5, ("conv5x5_split_kernel<32, 1, 2>",) + _KW),
    # 5x5 fp32 direct kernels: sliced below 1024 workgroups, whole above; f16x3 falls back where the split kernel does not apply
    NetCase("net_f16x3_5x5_dgrad_fallback", "f16x3", 2, 16, 12, 8, 16, 5,
            ("conv5x5_split_kernel<16, 1, 2>", "convk_direct_sliced_kernel<5, 16, 4>(dgrad)") + _KW),
    NetCase("net_f32_5x5_sliced_odd", "f32", 3, 5, 7, 11, 13, 5,
            ("convk_direct_sliced_kernel<5, 16, 4>", "convk_direct_sliced_kernel<5, 16, 4>(dgrad)") + _KW),
    NetCase("net_f32_5x5_direct_fwd", "f32", 64, 8, 64, 32, 32, 5, ("convk_direct_kernel<5, 16, 1>", "convk_direct_sliced_kernel<5, 16, 4>(dgrad)") + _KW),
    NetCase("net_bf16x6_5x5_direct_dgrad", "bf16x6", 64, 64, 8, 32, 32, 5,
            ("convk_direct_sliced_kernel<5, 16, 4>", "convk_direct_kernel<5, 16, 1>(dgrad)") + _KW),
]
BY_NAME.update({c.name: c for c in NET_CASES})


# ---------------------------------------------------------------- inputs, float64 reference, bound
U = 2.0 ** -24
# |y - y64| <= U * (C_MODE[mode] * A + [f16x3] C16 * M) + U * |extra|, per element; A = the operation on |operands|, M = max|a| * op(1, |b|)
# + max|b| * op(|a|, 1), extra = the bias (forward) or the whole accumulated result (weight gradient: gw0 + sum, rounded once more).
#  - fp32 accumulation of K products: each add rounds with |delta| <= U/2 relative to a partial sum, and partial sums of random-sign
#    products stay far below A.  Measured with torch's float32 CPU convolution (forward, unit-variance x, weights ~ U(-1, 1) / sqrt(fan-in)):
#    at most 3.9 U A over five shapes from Cin 8 to 128 (the largest at small Cin); test_bound_accepts_... re-measures five of the table's
#    forward shapes (0.24 - 0.65 of this bound).  8 = about twice the largest measured.
#  - bf16x6: three 8-bit terms per operand, the six products of order < 3; the dropped ones (x1 w2, x2 w1, x2 w2) and the
#    residual past x2 are each <= 2^-27 |x||w|: together < U/2 per product, inside the accumulation allowance.  Dropping the three
#    products of order 2 (x0 w2, x1 w1, x2 w0: each up to 2^-18 |x||w|) costs 15-70 U A: rejected.
#  - f16x3: 11-bit terms of operands scaled into [2^14, 2^15): the dropped x1 w1 and the rounding of each low term are <= 2^-22 |x||w|
#    per product (4 U), random in sign like the accumulation errors; +2 over the fp32 allowance.  A low term below fp16's normal range
#    (scaled |x| < 2^-3) may lose up to 2^-25 of the scaled maximum (>= 2^14): relative to max|x| that is 2^-39, flushed to zero 2^-28 -
#    C16 = 2 x 2^-28 / 2^-24 = 1/8 covers both operands even if the MFMA flushes fp16 subnormal inputs.  A missing cross product costs
#    2^-11 relative (> 900 U A): rejected.
C_MODE = {"f32": 8.0, "bf16x6": 8.0, "f16x3": 10.0}
C16 = 0.125


def inputs(case):
    """x (the layer input; H/2 x W/2 when up), w, bias, dy and the accumulated weight gradient gw0, float32, seeded by the case name"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    h, w = (case.H // 2, case.W // 2) if case.up else (case.H, case.W)
    x = rng.standard_normal((case.B, case.Cin, h, w), dtype=np.float32)
    k = getattr(case, "ksz", 3)
    wt = (rng.uniform(-1, 1, (case.Cout, case.Cin, k, k)) / math.sqrt(case.Cin * k * k)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, case.Cout).astype(np.float32)
    dy = rng.standard_normal((case.B, case.Cout, case.H, case.W), dtype=np.float32)
    gw0 = rng.uniform(-1, 1, (case.Cout, case.Cin, k, k)).astype(np.float32) if case.op != "net" else np.zeros((case.Cout, case.Cin, k, k), np.float32)
    return x, wt, b, dy, gw0


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def up2(x):
    """nearest x2 up-sampling of a float64 torch tensor"""
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def op64(op, a, b, shape):
    """float64 torch: op(a, b) for 'fwd' (a = x, b = w), 'dgrad' (a = dy, b = w), 'wgrad' (a = x, b = dy; shape = w's)"""
    import torch
    F = torch.nn.functional
    pad = shape[-1] // 2
    if op == "fwd":
        return F.conv2d(a, b, padding=pad)
    if op == "dgrad":
        return F.conv_transpose2d(a, b, padding=pad)
    return torch.nn.grad.conv2d_weight(a, shape, b, padding=pad)


def reference(case, x, w, b, dy, gw0, op=None, a_scale=None, b_scale=None):
    """(ref, bound) as float64 numpy arrays for the case's operation (op: one of the three when the case is a net case).  a_scale / b_scale:
    the magnitude the f16x3 kernel scales its first / second operand by (op64's a, b) where that is not the tensor's own maximum - an
    operand-ready (P16) image is scaled by an a-priori bound of its tensor (tests/p16_paths.py); default: the maximum, as the split kernels take it"""
    import torch
    op = op or case.op
    X, Wt, D = _t(x), _t(w), _t(dy)
    if case.up:
        X = up2(X)
    if op == "fwd":
        a, bb = X, Wt
    elif op == "dgrad":
        a, bb = D, Wt
    else:
        a, bb = X, D
    ref = op64(op, a, bb, tuple(w.shape))
    A = op64(op, a.abs(), bb.abs(), tuple(w.shape))
    bound = C_MODE[case.mode] * A
    if case.mode == "f16x3":
        sa = float(a.abs().max()) if a_scale is None else float(a_scale)
        sb = float(bb.abs().max()) if b_scale is None else float(b_scale)
        M = sa * op64(op, torch.ones_like(a), bb.abs(), tuple(w.shape)) + sb * op64(op, a.abs(), torch.ones_like(bb), tuple(w.shape))
        bound = bound + C16 * M
    if op == "fwd":
        ref = ref + _t(b)[None, :, None, None]
        bound = bound + _t(b).abs()[None, :, None, None]
    elif op == "wgrad":
        ref = ref + _t(gw0)
        bound = bound + ref.abs()
    return ref.numpy(), (U * bound).numpy()


def check_bound(got, ref, bound, what):
    """Every element within its bound; returns max |err| / bound (reported by the tests)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = err / bound
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert np.all(err <= bound), (f"{what}: {int((err > bound).sum())} of {err.size} elements outside u * (c A + ...); worst at {worst}: "
                                  f"got {float(np.asarray(got)[worst])!r}, float64 {ref[worst]!r}, bound {bound[worst]:.3e} (x{ratio[worst]:.1f})")
    return float(ratio[worst])


# ---------------------------------------------------------------- CPU emulations of the split arithmetic (test_conv_paths_host.py)
def split_terms_bf16(t, n=3):
    import torch
    out, r = [], t
    for _ in range(n):
        h = r.to(torch.bfloat16).float()
        out.append(h)
        r = r - h
    return out


def split_terms_f16(t, n=2):
    """scaled by a power of two into [2^14, 2^15) (f16_scale_exp), then split into fp16 terms"""
    s = 2.0 ** (14 - math.floor(math.log2(float(t.abs().max()))))
    out, r = [], t * s
    for _ in range(n):
        h = r.half().float()
        out.append(h)
        r = r - h
    return out, s


EMULATIONS = {          # name -> (split, products kept as (i, j) term pairs)
    "bf16x6": ("bf16", [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]),
    "bf16x6_without_order2": ("bf16", [(1, 0), (0, 1), (0, 0)]),
    "f16x3": ("f16", [(1, 0), (0, 1), (0, 0)]),
    "f16x3_without_x1w0": ("f16", [(0, 1), (0, 0)]),
    "fp16_single_term": ("f16", [(0, 0)]),
}


def emulate_forward(kind, x, w, b):
    """Forward convolution as a split kernel computes it: exact products of the terms, fp32 accumulation (torch's float32 conv2d of the
    term tensors), the products added in fp32 smallest first; 'fp32' = torch float32 conv2d.  float32 numpy result."""
    import torch
    F = torch.nn.functional
    X, Wt, bb = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)
    if kind == "fp32":
        return (F.conv2d(X, Wt, padding=1) + bb[None, :, None, None]).numpy()
    split, pairs = EMULATIONS[kind]
    if split == "bf16":
        xs, ws, scale = split_terms_bf16(X), split_terms_bf16(Wt), 1.0
    else:
        (xs, sx), (ws, sw) = split_terms_f16(X), split_terms_f16(Wt)
        scale = sx * sw
    y = None
    for i, j in pairs:
        p = F.conv2d(xs[i], ws[j], padding=1)
        y = p if y is None else y + p
    return (y / scale + bb[None, :, None, None]).numpy()
