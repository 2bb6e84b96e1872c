"""The operand-ready (P16) 3x3 convolution kernels of csrc/conv.hip - conv3x3_p16_quad_kernel, conv3x3_p16_quad_po_kernel, conv3x3_p16_k32_kernel,
conv3x3_wgrad_p16_pp_kernel, conv3x3_wgrad_reduce_tiled_kernel, conv3x3_fewin_p16o_kernel - and the part of csrc/net.hip that routes a stage onto
them, restated; two case tables (training-mode producer / consumer pairs, evaluate()-mode chains) that reach every leaf and every tile, chunk and
numbering edge; a float64 reference with a per-element bound; CPU emulations of the P16 arithmetic.

Used by tests/test_p16_paths_host.py (CPU: the tables reach every leaf and edge, the hand-written expectations equal the mirror, every case is on
the path its name claims, the bound accepts correct emulations and rejects degraded ones) and tests/test_gpu_p16_paths.py (the consumer's raw
output against a float64 convolution of the producer's output, every other observable as test_gpu_post_paths.py checks it, lean and timed reruns
bit for bit, labels against the mirror; the evaluate() chains against a propagated bound with the hand-over on and off).

A P16 image holds a tensor as two fp16 term planes per 8-channel group, scaled by a power of two taken from an A-PRIORI BOUND Bd of the tensor
(the kernel that writes the image cannot know the tensor's maximum before it has written it): the bound is folded from the statistics the stage
already has (elem.hip bn_stats_finalize_tiles_kernel, conv.hip eval_bound_kernel) and restated here in float64 (bound_fwd, bound_dy,
eval_bound).  Everything else of the arithmetic is the f16x3 split of conv_paths: three products x0 w0, x0 w1, x1 w0 accumulated in fp32.

THE BOUND.  u = 2^-24.  A convolution: conv_paths.reference's u (C_MODE["f16x3"] A + C16 M) + u |extra| with one difference - M, the allowance for a
low term that leaves fp16's normal range, is taken at Bd for an operand that arrives as a P16 image (reference's a_scale / b_scale), not at the
tensor's maximum: an image scaled at 2^k times its maximum flushes low terms 2^k times as large.  Bd is restated from the device's own raw
outputs and parameters and multiplied by BD_SLACK = 1 + 2^-10, so that the restatement is an upper estimate of the slot the device holds.
evaluate(): the handed-over tensors are not observable, so a bound E is carried along the float64 chain (eval_chain): few-input VALU convolution
(9 c0 + 1) u A; BatchNorm on running statistics and the activation as post_paths (E_z with the input's E in the place of E_mean, act_bound: only
Lipschitz constants, no decision is conditioned - every activation is continuous); the P16 quantisation of what is handed over 2^-22 |v| + 2^-39
Bd; the next convolution its own arithmetic bound plus conv64(E, |w|)."""
import dataclasses
import functools
import math
import types

import numpy as np

import conv_paths as cp
import post_paths as pp

U = 2.0 ** -24
BD_SLACK = 1.0 + 2.0 ** -10
Q_REL, Q_ABS = 2.0 ** -22, 2.0 ** -39      # P16 quantisation: two 11-bit terms; a low term below fp16's range, relative to the image's scale magnitude
MODE = "f16x3"

# ---------------------------------------------------------------- labels, as kernel_times() prints them
K32 = "conv3x3_p16_k32_kernel<16>"
REDUCE_TILED = "conv3x3_wgrad_reduce_tiled_kernel"


def quad_label(TW, NI, NG, MT, po=False):
    return f"conv3x3_p16_quad{'_po' if po else ''}_kernel<{TW}, {NI}, {NG}, {MT}>"


def pp_label(W):
    """launch_conv3x3_wgrad_p16 (conv.hip): FREE-running halves from 32-wide planes on"""
    return f"conv3x3_wgrad_p16_pp_kernel<{W}, {'true' if W >= 32 else 'false'}>"


def fewin_p16o_label(c0):
    return f"conv3x3_fewin_p16o_kernel<{c0}>"


QUADS = ((16, 1, 2, 1), (16, 2, 4, 2), (32, 1, 4, 2))
P16_LEAVES = frozenset({quad_label(*q, po=po) for q in QUADS for po in (False, True)} | {K32, REDUCE_TILED}
                       | {pp_label(W) for W in (16, 32, 64)} | {fewin_p16o_label(c) for c in (1, 2, 3)})


# ---------------------------------------------------------------- conv.hip, restated
def quad_geometry(TW, NI, NG, MT, B, Cin, Cout, H, W):
    """launch_conv_p16_quad<TW, NI, NG, MT> (conv.hip): tiles of PT = 128 NG pixels (NI whole images when NI > 1) x CT = 32 MT output channels,
    the input in 16-channel chunks"""
    PT, CT = 128 * NG, 32 * MT
    TR = PT // TW
    tiles_x, tiles_y = (W + TW - 1) // TW, 1 if NI > 1 else (H + TR - 1) // TR
    cout_pad = cp.round_up(Cout, 32)
    n_otiles = cout_pad // CT
    n_tiles = ((B + NI - 1) // NI) * tiles_x * tiles_y * n_otiles
    return dict(kind="quad", T=(TW, NI, NG, MT), tiles_x=tiles_x, tiles_y=tiles_y, n_otiles=n_otiles, n_tiles=n_tiles, grid=n_tiles, CT=CT,
                cout_pad=cout_pad, real_last=Cout - (n_otiles - 1) * CT, chunks=Cin // 16, B=B, NI=NI)


def k32_geometry(TW, B, Cin, Cout, H, W):
    """launch_conv_p16_k32<TW> (conv.hip): 256-pixel x 32-channel units, 32-channel chunks, at most 512 resident workgroups walk the units"""
    TR = 256 // TW
    tiles_x, tiles_y = (W + TW - 1) // TW, (H + TR - 1) // TR
    cout_pad = cp.round_up(Cout, 32)
    n_otiles = cout_pad // 32
    n_tiles = B * tiles_x * tiles_y * n_otiles
    return dict(kind="k32", T=(TW,), tiles_x=tiles_x, tiles_y=tiles_y, n_otiles=n_otiles, n_tiles=n_tiles, grid=min(n_tiles, 512), CT=32,
                cout_pad=cout_pad, real_last=Cout - (n_otiles - 1) * 32, chunks=Cin // 32, B=B, NI=1)


def conv_p16_launch(B, Cin, Cout, H, W, plain_out, po=False):
    """launch_conv3x3_p16 (conv.hip) -> (label, geometry).  plain_out: no fused epilogue, no operand-ready output, an fp32 destination (training
    mode and every data gradient); po: the result leaves operand-ready (evaluate())"""
    assert not (plain_out and po)
    two_img_tiles = ((B + 1) // 2) * (cp.round_up(Cout, 32) // 64)
    if H == 16 and W == 16 and two_img_tiles < 512 and Cin % 32 == 0 and plain_out:
        return K32, dict(k32_geometry(16, B, Cin, Cout, H, W), two_img_tiles=two_img_tiles)
    if H == 16 and W == 16:
        q = (16, 1, 2, 1) if two_img_tiles < 512 else (16, 2, 4, 2)
    else:
        q = (32, 1, 4, 2)
    g = quad_geometry(*q, B, Cin, Cout, H, W)
    g["two_img_tiles"] = two_img_tiles
    return quad_label(*q, po=po), g


def wgrad_p16_splits(B, Cin, Cout, H, W):
    """conv.hip wgrad_p16_splits: one eight-wave workgroup per CU over the (Cin / 64) x (Cout / 64) blocks, at most one per 64-pixel chunk"""
    blocks = (Cin // 64) * (Cout // 64)
    return min(max(256 // blocks, 1), B * H * W // 64)


def wgrad_p16_xcd_numbering(n_cb, n_ob, nsplit):
    """wgrad_p16_block's test: the combinations of a split 8 block ids apart (the same XCD)"""
    return n_cb * n_ob > 1 and nsplit % 8 == 0


def wgrad_p16_block(n_cb, n_ob, nsplit, bid):
    """conv.hip wgrad_p16_block, both numberings -> (cb, ob, split)"""
    C = n_cb * n_ob
    if wgrad_p16_xcd_numbering(n_cb, n_ob, nsplit):
        grp = bid // (8 * C)
        rem = bid - grp * 8 * C
        combo = rem >> 3
        return combo % n_cb, combo // n_cb, grp * 8 + (rem & 7)
    cb = bid % n_cb
    bid //= n_cb
    return cb, bid % n_ob, bid // n_ob


def wgrad_p16_launch(B, Cin, Cout, H, W):
    """launch_conv3x3_wgrad_p16 + the kernel's run arithmetic (conv3x3_wgrad_p16_pp_kernel: w0, w1, wm) -> geometry.  runs: per split the
    (half A, half B) chunk counts"""
    n_ob, n_cb = Cout // 64, Cin // 64
    nsplit, units = wgrad_p16_splits(B, Cin, Cout, H, W), B * H * W // 64
    runs = []
    for split in range(nsplit):
        w0, w1 = split * units // nsplit, (split + 1) * units // nsplit
        wm = w0 + (w1 - w0 + 1) // 2
        runs.append((wm - w0, w1 - wm))
    return dict(label=pp_label(W), n_ob=n_ob, n_cb=n_cb, nsplit=nsplit, units=units, grid=nsplit * n_ob * n_cb, runs=runs,
                xcd=wgrad_p16_xcd_numbering(n_cb, n_ob, nsplit), chunks_per_image=H * W // 64, rows_per_chunk=max(64 // W, 1),
                reduce_grid=(9 * Cout * Cin // 4 + 31) // 32)


def fewin_og(grid, Cout, p16_out):
    """launch_conv3x3_fewin's output-channel slices `og`: doubled towards 1024 workgroups while a slice keeps >= 8 channels (operand-ready
    output: whole 8-channel groups)"""
    og = 1
    while grid * og < 1024 and Cout // (2 * og) >= 8 and (not p16_out or Cout % (16 * og) == 0):
        og *= 2
    return og


def fewin_geometry(B, c0, Cout, H, W, p16_out):
    tiles_x, tiles_y = (W + 31) // 32, (H + 31) // 32
    grid = B * tiles_x * tiles_y
    og = fewin_og(grid, Cout, p16_out)
    return dict(kind="fewin", tiles_x=tiles_x, tiles_y=tiles_y, grid=grid, og=og, o_per=(Cout + og - 1) // og, H=H, W=W)


def fewin_p16_out_supported(Cout, H, W):
    """conv.hip conv_fewin_p16_out_supported"""
    return Cout % 8 == 0 and Cout <= 256 and W % 4 == 0


# ---------------------------------------------------------------- net.hip, restated: training mode
@dataclasses.dataclass(frozen=True)
class TrainCase:
    """f16x3, p16_min_tiles = 1, training: conv(1 -> C1) + `layers` (the producer: BatchNorm, ELU / Sigmoid / Tanh, optionally an average pool and a
    Dropout - no discrete decision anywhere), then conv(C1 -> C2) + BatchNorm (the consumer).  H x W: the producer's plane.  fwd: the consumer
    convolution's forward leaf; bwd: the P16 leaves of the backward (data gradient, weight gradient + its reduction), hand-written."""
    name: str
    B: int
    C1: int
    C2: int
    H: int
    W: int
    layers: tuple
    fwd: str
    bwd: tuple = ()
    backward: bool = True      # False: forward only (the float64 gradients of B = 130 / B = 63 x 1024 channels would cost minutes)

    @property
    def stage(self):
        return pp.stage_of(self.layers, True)

    @property
    def out_hw(self):
        return (self.H // 2, self.W // 2) if self.stage.pool != "none" else (self.H, self.W)

    def expect(self):
        return {self.fwd: 1}, ({k: 1 for k in self.bwd} if self.backward else {})

    def mirror(self):
        r = train_route(self)
        fwd = {r.fwd[0]: 1} if r.in_p16 else {}
        bwd = {}
        if self.backward:
            if r.dgrad:
                bwd[r.dgrad[0]] = 1
            if r.wgrad:
                bwd[r.wgrad["label"]] = 1
                bwd[REDUCE_TILED] = 1
        return fwd, bwd


def train_route(c, min_tiles=1, guarded=True):
    """net.hip forward_stages / fwd_conv3 / fwd_post / backward_impl for a TrainCase (p16_input_ok, in_p16, p16_dy_ok, p16_wgrad_ok, dgrad_p16,
    wgrad_p16, out_skipped) -> namespace(in_p16, fwd = (label, geometry), dgrad = (label, geometry) or None, wgrad = geometry or None, lean,
    p1, p2 = the two stages' post_paths.Plan)"""
    f1, f2 = c.stage, pp.Stage(bn=True)
    pool = f1.pool != "none"
    H2, W2 = c.out_hw
    # p16_input_ok(consumer): the image buffer exists (ensure_batch: Cin % 16 == 0) and conv_p16_supported
    p16_in2 = c.C1 % 16 == 0 and pp.conv_p16_supported(c.B, c.C1, c.C2, H2, W2, min_tiles)
    tiles1 = pp.conv_stat_tiles(MODE, c.B, 1, c.C1, c.H, c.W)
    # fwd_post: p16_out only on the statistics-tile route (the a-priori bound is folded there)
    p16_out1 = f1.bn and tiles1 > 0 and p16_in2 and pp.post_g8_supported(c.C1, c.H, c.W, pool)
    in_p16 = p16_out1                                   # fwd_conv3: x_p16_gen current
    fwd = conv_p16_launch(c.B, c.C1, c.C2, H2, W2, plain_out=True) if in_p16 else (cp.split_leaf(2, c.B, c.C2, H2, W2, False, 128), None)
    tiles2 = pp.conv_stat_tiles(MODE, c.B, c.C1, c.C2, H2, W2, in_p16=in_p16)
    g8_dy = pp.post_g8_supported(c.C2, H2, W2, False, True)
    dy_ok2 = tiles2 > 0 and g8_dy                       # kb_gen current (the tile route ran) and p16_dy_ok
    wgrad_ok2 = g8_dy and c.C1 % 16 == 0 and pp.conv_wgrad_p16_supported(c.B, c.C1, c.C2, H2, W2)      # p16_wgrad_ok
    dgrad_p16 = dy_ok2 and pp.conv_p16_supported(c.B, c.C2, c.C1, H2, W2, min_tiles)                    # (need_gin: the consumer is not the first stage)
    wgrad_p16 = dy_ok2 and p16_out1 and wgrad_ok2
    p1 = pp.plan(f1, True, c.B, c.C1, c.H, c.W, "conv", tiles1, p16_out=p16_out1)
    p2 = pp.plan(f2, True, c.B, c.C2, H2, W2, "conv", tiles2, dy_p16=dgrad_p16 or wgrad_p16)
    return types.SimpleNamespace(in_p16=in_p16, fwd=fwd, lean=(not guarded) and p16_out1 and wgrad_ok2, p1=p1, p2=p2,
                                 dgrad=conv_p16_launch(c.B, c.C2, c.C1, H2, W2, plain_out=True) if dgrad_p16 else None,
                                 wgrad=wgrad_p16_launch(c.B, c.C1, c.C2, H2, W2) if wgrad_p16 else None)


_Q1, _Q2, _Q32 = quad_label(16, 1, 2, 1), quad_label(16, 2, 4, 2), quad_label(32, 1, 4, 2)
_PLAIN, _DROP, _AVG = ("bn", "ELU"), ("bn", "ELU", "drop"), ("bn", "Tanh", "avg")
TRAIN_CASES = [
    # ---- forward edges (B, C1, C2, the consumer's plane)
    TrainCase("k32_one_chunk_ragged_xcd", 3, 32, 64, 16, 16, _DROP, K32),                          # 6 units: not a multiple of 8 (xcd_remap ragged); C1 = 32: no P16 gradient
    TrainCase("k32_three_chunks_padded_out", 2, 96, 40, 16, 16, ("bn", "Sigmoid"), K32),           # 40 of 64 output channels
    TrainCase("k32_second_unit_b130", 130, 32, 128, 16, 16, _PLAIN, K32, backward=False),          # 520 units over 512 workgroups
    TrainCase("quad16_three_chunks_cout100", 3, 48, 100, 16, 16, _DROP, _Q1),                      # Cin % 32 != 0; 4 blocks of 32, the last with 4 real channels; 100 % 8: no g8 pass B
    TrainCase("quad16_one_chunk", 3, 16, 64, 16, 16, ("bn", "Tanh"), _Q1),
    TrainCase("quad16x2_512_tiles_odd_batch", 63, 16, 1024, 16, 16, _PLAIN, _Q2, backward=False),  # the last tile's second image absent
    TrainCase("quad16_511_two_image_tiles", 145, 16, 448, 16, 16, _PLAIN, _Q1, backward=False),       # 73 x 7: the last count below the two-image threshold
    TrainCase("k32_511_two_image_tiles", 145, 32, 448, 16, 16, _PLAIN, K32, backward=False),          # ... and k32's own test of the same count
    TrainCase("quad32_tiles_y2_padded_out", 1, 16, 40, 32, 32, _DROP, _Q32),
    TrainCase("quad32_tiles_x2", 2, 64, 64, 16, 64, _PLAIN, _Q32, (_Q32, pp_label(64), REDUCE_TILED)),
    TrainCase("quad32_tiles_y4_two_chunks", 1, 32, 64, 64, 32, ("bn", "Sigmoid"), _Q32),
    TrainCase("k32_behind_avg_pool", 3, 64, 64, 32, 32, _AVG, K32, (K32, pp_label(16), REDUCE_TILED)),    # the image is written at the pooled size
    # ---- data gradient: the channel roles exchanged (needs C2 % 16 == 0, round_up(C1, 32) % 64 == 0)
    TrainCase("dgrad_quad16_padded_48_48", 3, 48, 48, 16, 16, _DROP, _Q1, (_Q1,)),                 # as a data gradient: 48 of 64 output channels, three chunks
    # ---- weight gradient (C1 % 64 == 0, C2 % 64 == 0, W in 16 / 32 / 64)
    TrainCase("wgrad16_plain_numbering_two_blocks", 3, 128, 64, 16, 16, _DROP, K32, (K32, pp_label(16), REDUCE_TILED)),      # n_cb 2, nsplit 12
    TrainCase("wgrad16_xcd_numbering", 4, 64, 128, 16, 16, _PLAIN, K32, (K32, pp_label(16), REDUCE_TILED)),                  # n_ob 2, nsplit 16
    TrainCase("wgrad16_uneven_runs_idle_half", 17, 128, 128, 16, 16, _DROP, K32, (K32, pp_label(16), REDUCE_TILED)),         # 68 chunks over 64 splits
    TrainCase("wgrad32_non_square", 1, 64, 64, 16, 32, _PLAIN, _Q32, (_Q32, pp_label(32), REDUCE_TILED)),                    # eight chunks per image
    TrainCase("wgrad32_n_cb_3", 1, 192, 64, 32, 32, ("bn", "Tanh"), _Q32, (_Q32, pp_label(32), REDUCE_TILED)),
    TrainCase("wgrad64_16x64", 1, 64, 64, 16, 64, _DROP, _Q32, (_Q32, pp_label(64), REDUCE_TILED)),                          # one image row per chunk
    TrainCase("wgrad64_64x64", 1, 64, 64, 64, 64, ("bn", "Sigmoid"), _Q32, (_Q32, pp_label(64), REDUCE_TILED)),
]
TRAIN_BY_NAME = {c.name: c for c in TRAIN_CASES}


# ---------------------------------------------------------------- net.hip, restated: evaluate() mode
@dataclasses.dataclass(frozen=True)
class EvalCase:
    """f16x3, p16_min_tiles = 1, evaluate(): conv(c0 -> C[0]) + BN + ELU, then conv(C[i-1] -> C[i]) + BN + acts[i] (+ an average pool where
    pools[i]).  on / off: the convolution labels of a forward with eval_p16 = 1 / 0, in stage order, hand-written."""
    name: str
    B: int
    c0: int
    H: int
    W: int
    C: tuple
    acts: tuple
    on: tuple
    off: tuple
    pools: tuple = ()

    def stages(self):
        """(Cin, Cout, H, W, act, pool) per stage"""
        out, cin, h, w = [], self.c0, self.H, self.W
        for i, co in enumerate(self.C):
            pool = bool(self.pools) and self.pools[i]
            out.append((cin, co, h, w, self.acts[i], pool))
            cin = co
            if pool:
                h, w = h // 2, w // 2
        return out

    def mirror(self, eval_p16=1):
        return tuple(r["label"] for r in eval_route(self, eval_p16))


def eval_route(c, eval_p16=1, min_tiles=1):
    """net.hip fwd_conv3 / fwd_post for an EvalCase: per stage dict(label, geometry, in_p16, po, post_p16).  eval_epilogue fuses BatchNorm and
    the activation into the convolution unless the stage pools; nx_p16 / po / post_p16 as fwd_conv3 writes them."""
    st = c.stages()
    out, in_p16 = [], False
    for i, (cin, co, h, w, act, pool) in enumerate(st):
        nx = st[i + 1] if i + 1 < len(st) else None
        is_fewin = pp.conv_fewin_applies(cin, w)
        fused = not pool                                 # eval_epilogue: no pool, no PReLU, no active mask
        nx_in_ok = nx is not None and nx[0] % 16 == 0 and pp.conv_p16_supported(c.B, nx[0], nx[1], nx[2], nx[3], min_tiles)     # p16_input_ok(nx)
        nx_p16 = bool(eval_p16) and nx_in_ok
        po = nx_p16 and fused and (fewin_p16_out_supported(co, h, w) if is_fewin else (in_p16 and co % 8 == 0))
        post_p16 = nx_p16 and not fused and pp.post_g8_supported(co, h, w, pool)
        if is_fewin:
            label, geo = (fewin_p16o_label(cin) if po else f"conv3x3_fewin_kernel<{cin}>"), fewin_geometry(c.B, cin, co, h, w, po)
        elif in_p16:
            label, geo = conv_p16_launch(c.B, cin, co, h, w, plain_out=not fused and not po, po=po)
        else:
            label, geo = cp.split_leaf(2, c.B, co, h, w, False, 128), None
        out.append(dict(label=label, geo=geo, in_p16=in_p16, po=po, post_p16=post_p16, fused=fused))
        in_p16 = po or post_p16
    return out


_SP16, _SP16W = "conv3x3_split_kernel<16, 2, 2>", "conv3x3_split_wide_kernel<16, 2, 2, true>"
_SP32 = "conv3x3_split_kernel<32, 2, 2>"
_FI = "conv3x3_fewin_kernel<{}>".format
EVAL_CASES = [
    # two stages: the few-input kernel's operand-ready output is the subject (og, o_per, the tile edge), a quad kernel consumes it
    EvalCase("fewin1_og1_b1024", 1024, 1, 16, 16, (16, 40), ("ELU", "Tanh"), (fewin_p16o_label(1), _Q2), (_FI(1), _SP16W)),       # og = 1 needs 1024 workgroups: C1 % 16 == 0 doubles og below that
    EvalCase("fewin2_og2_o_per24", 3, 2, 16, 16, (48, 40), ("ELU", "Sigmoid"), (fewin_p16o_label(2), _Q1), (_FI(2), _SP16)),      # plane smaller than the 32 x 32 tile
    EvalCase("fewin3_og8_two_tile_rows", 2, 3, 64, 32, (64, 64), ("ELU", "LeakyReLU"), (fewin_p16o_label(3), _Q32), (_FI(3), _SP32)),
    # three stages: quad_po in the middle (padded output channels: 48 of 64 - the hand-over needs C2 % 16 == 0, so not 40), quad at the end
    EvalCase("po16_c48_c40", 3, 1, 16, 16, (16, 48, 40), ("ELU", "LeakyReLU", "Sigmoid"),
             (fewin_p16o_label(1), quad_label(16, 1, 2, 1, po=True), _Q1), (_FI(1), _SP16, _SP16)),
    EvalCase("po32_c48_c40", 1, 2, 32, 32, (32, 48, 40), ("ELU", "Sigmoid", "ELU"),
             (fewin_p16o_label(2), quad_label(32, 1, 4, 2, po=True), _Q32), (_FI(2), _SP32, _SP32)),
    EvalCase("po16x2_512_tiles", 63, 1, 16, 16, (16, 1024, 40), ("ELU", "ELU", "Tanh"),
             (fewin_p16o_label(1), quad_label(16, 2, 4, 2, po=True), _Q1), (_FI(1), _SP16W, _SP16)),                              # the module's most expensive float64 reference
    # the middle stage pools: no fused epilogue, so its convolution writes plain fp32 (quad<32>: a 32 x 32 plane) and its pipeline kernel the
    # image (post_p16); the last stage's fused epilogue keeps it off k32
    EvalCase("post_p16_avg_pool", 3, 1, 32, 32, (64, 64, 40), ("ELU", "Tanh", "Sigmoid"),
             (fewin_p16o_label(1), _Q32, _Q1), (_FI(1), _SP32, _SP16), pools=(False, True, False)),
]
EVAL_BY_NAME = {c.name: c for c in EVAL_CASES}


# ---------------------------------------------------------------- edges: name -> predicate over (case, route)
def _tr(f):
    """a predicate over training cases only (route = train_route's namespace)"""
    return lambda c, r: isinstance(c, TrainCase) and f(c, r)


def _ev(f):
    """a predicate over evaluate() cases only (route = eval_route's list)"""
    return lambda c, r: isinstance(c, EvalCase) and f(c, r)


def _launches(c, r):
    """every P16 convolution launch (label, geometry) of a case, forward and data gradient"""
    if isinstance(c, TrainCase):
        return ([r.fwd] if r.in_p16 else []) + ([r.dgrad] if r.dgrad and c.backward else [])
    return [(s["label"], s["geo"]) for s in r if s["geo"] is not None and s["geo"]["kind"] != "fewin"]


def _any(f):
    return lambda c, r: any(f(l, g) for l, g in _launches(c, r))


_wg = lambda f: _tr(lambda c, r: c.backward and r.wgrad is not None and f(r.wgrad))
EDGES = {
    "k32_one_chunk": _any(lambda l, g: l == K32 and g["chunks"] == 1),
    "k32_units_not_multiple_of_8": _any(lambda l, g: l == K32 and g["n_tiles"] % 8 != 0),
    "k32_second_unit": _any(lambda l, g: l == K32 and g["n_tiles"] > g["grid"] == 512),
    "half_empty_two_image_tile": _any(lambda l, g: g["kind"] == "quad" and g["NI"] == 2 and g["B"] % 2 == 1 and g["two_img_tiles"] >= 512),
    "two_image_threshold_from_below": _any(lambda l, g: l == _Q1 and g["two_img_tiles"] == 511),
    "two_image_threshold_from_below_k32": _any(lambda l, g: l == K32 and g["two_img_tiles"] == 511),
    "two_image_threshold_from_above": _any(lambda l, g: l == _Q2 and g["two_img_tiles"] == 512),
    "padded_output_block": _any(lambda l, g: g["real_last"] < g["CT"]),
    "padded_output_block_k32": _any(lambda l, g: l == K32 and g["real_last"] < 32),
    "padded_output_block_quad16": _any(lambda l, g: l == _Q1 and g["real_last"] < 32),
    "padded_output_block_quad32": _any(lambda l, g: l == _Q32 and g["real_last"] < 64),
    "padded_output_block_po": _any(lambda l, g: "_po_" in l and g["real_last"] < g["CT"]),
    "more_than_one_output_block": _any(lambda l, g: g["n_otiles"] > 1),
    "chunks_ge_3": _any(lambda l, g: g["chunks"] >= 3),
    "chunks_ge_3_quad_cin_not_32": _any(lambda l, g: g["kind"] == "quad" and g["chunks"] == 3),
    "quad_one_chunk": _any(lambda l, g: g["kind"] == "quad" and g["chunks"] == 1),
    "tiles_x_gt_1": _any(lambda l, g: g["tiles_x"] > 1),
    "tiles_y_gt_1": _any(lambda l, g: g["tiles_y"] > 1),
    "tiles_y_4": _any(lambda l, g: g["tiles_y"] == 4 and g["chunks"] == 2),
    "image_written_at_pooled_size": _tr(lambda c, r: r.in_p16 and c.stage.pool == "avg"),
    "dgrad_k32": _tr(lambda c, r: c.backward and r.dgrad is not None and r.dgrad[0] == K32),
    "dgrad_quad16": _tr(lambda c, r: c.backward and r.dgrad is not None and r.dgrad[0] == _Q1),
    "dgrad_quad32": _tr(lambda c, r: c.backward and r.dgrad is not None and r.dgrad[0] == _Q32),
    "dgrad_padded_output_block": _tr(lambda c, r: c.backward and r.dgrad is not None and r.dgrad[1]["real_last"] < r.dgrad[1]["CT"]),
    "wgrad_xcd_numbering": _wg(lambda g: g["xcd"]),
    "wgrad_plain_numbering_multi_block": _wg(lambda g: not g["xcd"] and g["n_ob"] * g["n_cb"] > 1),
    "wgrad_uneven_runs": _wg(lambda g: len({a + b for a, b in g["runs"]}) > 1),
    "wgrad_idle_half": _wg(lambda g: any(b == 0 for a, b in g["runs"])),
    "wgrad_reduce_n_ob_n_cb_2": _wg(lambda g: g["n_ob"] == 2 and g["n_cb"] == 2),
    "n_cb_not_pow2": _wg(lambda g: g["n_cb"] & (g["n_cb"] - 1) != 0),
    "wgrad32_non_square_8_chunks": _tr(lambda c, r: c.backward and r.wgrad is not None and r.wgrad["label"] == pp_label(32) and c.out_hw[0] != c.out_hw[1]
                                       and r.wgrad["chunks_per_image"] == 8),
    "wgrad64_one_row_per_chunk": _wg(lambda g: g["label"] == pp_label(64) and g["rows_per_chunk"] == 1),
    "lean_skips_the_producer_output": _tr(lambda c, r: train_route(c, guarded=False).lean),
    "fewin_og_1": _ev(lambda c, r: r[0]["po"] and r[0]["geo"]["og"] == 1),
    "fewin_og_gt_1": _ev(lambda c, r: r[0]["po"] and r[0]["geo"]["og"] > 1),
    "fewin_og_2_o_per_24": _ev(lambda c, r: r[0]["po"] and r[0]["geo"]["og"] == 2 and r[0]["geo"]["o_per"] == 24),
    "fewin_og_8": _ev(lambda c, r: r[0]["po"] and r[0]["geo"]["og"] == 8),
    "fewin_plane_below_tile": _ev(lambda c, r: r[0]["po"] and r[0]["geo"]["H"] < 32 and r[0]["geo"]["W"] < 32),
    "fewin_two_tile_rows": _ev(lambda c, r: r[0]["po"] and r[0]["geo"]["tiles_y"] == 2),
    "eval_post_p16_behind_pool": _ev(lambda c, r: any(s["post_p16"] for s in r)),
    "eval_quad_po_512_two_image_tiles": _ev(lambda c, r: any(s["po"] and s["geo"]["kind"] == "quad" and s["geo"]["NI"] == 2 and s["geo"]["n_tiles"] == 512 for s in r)),
}


def route(c):
    return train_route(c) if isinstance(c, TrainCase) else eval_route(c)


# ---------------------------------------------------------------- the a-priori bounds, restated in float64
def _chan(y):
    y = np.asarray(y, np.float64)
    n = y.shape[0] * y.shape[2] * y.shape[3]
    m = y.mean((0, 2, 3))
    var = ((y - m[None, :, None, None]) ** 2).mean((0, 2, 3))
    return n, m, 1.0 / np.sqrt(var + pp.EPS)


def _mask_factor(f):
    """net.hip fwd_post: fmaxf(1, m1.scale) * fmaxf(1, m2.scale)"""
    return max(1.0, pp.mask_scale(f.m1)) * max(1.0, pp.mask_scale(f.m2))


def bound_fwd(f, y, gamma, beta):
    """elem.hip bn_stats_finalize_tiles_kernel's bound_out: max_c ((ymax + |mean_c|) invstd_c |gamma_c| + |beta_c|), at most 1 behind Sigmoid / Tanh,
    x the masks' scale x 1.0001; y = the stage's raw convolution output (the device's).  x BD_SLACK"""
    _, m, invstd = _chan(y)
    zb = (float(np.abs(y).max()) + np.abs(m)) * invstd * np.abs(gamma.astype(np.float64)) + np.abs(beta.astype(np.float64))
    if f.act in ("Sigmoid", "Tanh"):
        zb = np.minimum(zb, 1.0)
    return float(zb.max()) * _mask_factor(f) * 1.0001 * BD_SLACK


def bound_dy(y, gamma, dz_max):
    """elem.hip: kb_out = max_c (2 + (ymax + |mean_c|) invstd_c) invstd_c |gamma_c| x 1.0001; pass B scales the dy image by max|dz| x kb.  x BD_SLACK"""
    _, m, invstd = _chan(y)
    kb = (2.0 + (float(np.abs(y).max()) + np.abs(m)) * invstd) * invstd * np.abs(gamma.astype(np.float64)) * 1.0001
    return float(dz_max) * float(kb.max()) * BD_SLACK


def eval_bound(in_max, w, b, gamma, beta, rm, rv, act, slope, post_scale=1.0):
    """conv.hip eval_bound_kernel.  w given (a fused epilogue hands over): per-channel L1 weight norm (conv_weight_l1_kernel: x 1.000001) x the TRUE
    maximum of the stage input + |bias|; w None (a pipeline kernel hands over): in_max = max|y| of the raw output.  Then the running-statistics
    affine map on magnitudes, the activation's bound, x post_scale x 1.001.  x BD_SLACK"""
    f8 = lambda t: np.asarray(t, np.float64)
    v = np.full(len(gamma), float(in_max)) if w is None else np.abs(f8(w)).sum((1, 2, 3)) * 1.000001 * float(in_max) + np.abs(f8(b))
    invstd = 1.0 / np.sqrt(f8(rv) + pp.EPS)
    v = (v + np.abs(f8(rm))) * invstd * np.abs(f8(gamma)) + np.abs(f8(beta))
    if act in ("Sigmoid", "Tanh"):
        v = np.minimum(v, 1.0)
    elif act == "LeakyReLU":
        v = v * max(1.0, abs(float(slope)))
    return float(v.max()) * post_scale * 1.001 * BD_SLACK


# ---------------------------------------------------------------- inputs
def train_inputs(c):
    """x (B, 1, H, W), the two convolutions' weights and biases, the two stages' parameters, masks and gradOutput (post_paths.stage_inputs with y left
    to the device), seeded by the case name"""
    rng = pp._rng(f"{c.name} p16 main")
    x = rng.standard_normal((c.B, 1, c.H, c.W), dtype=np.float32)
    w1 = (rng.uniform(-1, 1, (c.C1, 1, 3, 3)) / 3.0).astype(np.float32)
    b1 = rng.uniform(-0.5, 0.5, c.C1).astype(np.float32)
    w2 = (rng.uniform(-1, 1, (c.C2, c.C1, 3, 3)) / np.sqrt(9.0 * c.C1)).astype(np.float32)
    b2 = rng.uniform(-0.5, 0.5, c.C2).astype(np.float32)
    H2, W2 = c.out_hw
    z = lambda *s: np.zeros(s, np.float32)
    d1 = pp.stage_inputs(f"{c.name} p16 1", c.stage, True, c.B, c.C1, c.H, c.W, y=z(1))
    d2 = pp.stage_inputs(f"{c.name} p16 2", pp.Stage(bn=True), True, c.B, c.C2, H2, W2, y=z(1))
    return x, w1, b1, w2, b2, d1, d2


@functools.lru_cache(maxsize=None)
def eval_inputs(name):
    """x (B, c0, H, W) and per stage (w, b, gamma, beta, running mean, running variance), float32, read-only (the tests share them)"""
    c = EVAL_BY_NAME[name]
    rng = pp._rng(f"{name} p16 eval")
    x = rng.standard_normal((c.B, c.c0, c.H, c.W), dtype=np.float32)
    params = []
    for cin, co, h, w, act, pool in c.stages():
        wt = (rng.uniform(-1, 1, (co, cin, 3, 3)) / np.sqrt(3.0 * cin)).astype(np.float32)          # y of about unit variance on unit-variance inputs
        b = rng.uniform(-0.5, 0.5, co).astype(np.float32)
        gamma = (rng.uniform(0.5, 1.5, co) * np.where(np.arange(co) % 2, -1.0, 1.0)).astype(np.float32)
        beta = rng.uniform(-0.5, 0.5, co).astype(np.float32)
        rm, rv = rng.uniform(-0.3, 0.3, co).astype(np.float32), rng.uniform(0.6, 1.6, co).astype(np.float32)
        params.append((wt, b, gamma, beta, rm, rv))
    for t in (x,) + tuple(a for p in params for a in p):
        t.setflags(write=False)
    return x, tuple(params)


# ---------------------------------------------------------------- float64 references
_NS = {op: types.SimpleNamespace(mode=MODE, up=False, op=op) for op in ("fwd", "dgrad", "wgrad")}


def conv_ref(op, x, w, b, dy, a_scale=None, b_scale=None, E_a=None, E_b=None):
    """(float64 reference, bound) of one convolution in f16x3 arithmetic: conv_paths.reference with the P16 operands' scale magnitudes, plus the
    operands' own bounds E_a / E_b (op64's a, b) carried through the magnitudes of the other operand.  wgrad: gradWeight accumulated onto zero."""
    nob = np.zeros(w.shape[0], np.float32) if b is None else b
    zero = np.zeros(w.shape, np.float32)
    if op == "fwd":
        dy = np.zeros((1, w.shape[0], 1, 1), np.float32)
    elif op == "dgrad":
        x = np.zeros((1, w.shape[1], 1, 1), np.float32)
    ref, bound = cp.reference(_NS[op], x, w, nob, dy, zero, a_scale=a_scale, b_scale=b_scale)
    a, bb = (x, w) if op == "fwd" else (dy, w) if op == "dgrad" else (x, dy)
    if E_a is not None:
        bound = bound + cp.op64(op, cp._t(E_a), cp._t(bb).abs(), w.shape).numpy()
    if E_b is not None:
        bound = bound + cp.op64(op, cp._t(a).abs(), cp._t(E_b), w.shape).numpy()
    return ref, bound


def bn_act64(y, Ey, gamma, beta, rm, rv, act, slope, pool):
    """evaluate()-mode BatchNorm (running statistics) + activation (+ 2 x 2 average pool) in float64 with post_paths' bounds; Ey: the bound of y,
    which takes the place of E_mean in E_z.  -> (out, E_out)"""
    ch = lambda t: np.asarray(t, np.float64)[None, :, None, None]
    invstd = 1.0 / np.sqrt(np.asarray(rv, np.float64) + pp.EPS)
    c = y - ch(rm)
    z = c * ch(invstd) * ch(gamma) + ch(beta)
    Ez = np.abs(ch(gamma) * ch(invstd)) * (Ey + np.abs(c) * (3 * U + U)) + U * np.abs(z)       # (r_inv = u: invstd rounded from an fp64 value)
    a = pp.act64(act, z, slope)
    Ea = pp.act_bound(act, z, a, Ez, slope)
    if pool:
        w, Ew = pp._windows(a), pp._windows(Ea)
        a, Ea = w.sum(-1) / 4, (Ew.sum(-1) + 3 * U * np.abs(w).sum(-1)) / 4
    return a, pp.SLACK * Ea


def eval_chain(c, x, params, slope=pp.LEAKY_SLOPE):
    """The evaluate() chain of an EvalCase in float64 with the propagated per-element bound -> (out, E, [Bd of each hand-over], [(y, E_y) of each
    stage's raw convolution output: observable where the stage pools, i.e. has no fused epilogue]).  The same bound serves eval_p16 = 0: without
    the hand-over the quantisation terms are slack, and the split kernels scale by the true maximum <= Bd.
    HOW TIGHT.  E passes a convolution as conv64(E, |w|): it grows by sum|w| where independent roundings grow by its root, about 20 x per stage
    at 64 channels.  MEASURED (test_p16_paths_host.py, single-term hand-overs): behind ONE hand-over the bound is exceeded 8-10 x, behind two
    (48 channels) 2-3 x, behind two with a 576- or 9216-term last convolution the output stays at 0.5-0.8 of it.  So the two-stage chains and the
    raw output of a pooling stage guard the low-order products; the last stage of the two widest chains guards tiles, chunks and channel blocks
    (errors of the size of the result), as does every case."""
    st = c.stages()
    v, E, Bd, bds, raws = x.astype(np.float64), None, None, [], []
    true_max = float(np.abs(v).max())
    for i, ((cin, co, h, w_, act, pool), (wt, b, gamma, beta, rm, rv)) in enumerate(zip(st, params)):
        if i == 0:       # few-input VALU convolution: 9 c0 FMAs and the bias, fp32
            X, Wt = cp._t(v), cp._t(wt)
            y = cp.op64("fwd", X, Wt, wt.shape).numpy() + b.astype(np.float64)[None, :, None, None]
            A = cp.op64("fwd", X.abs(), Wt.abs(), wt.shape).numpy() + np.abs(b.astype(np.float64))[None, :, None, None]
            Ey = (9 * cin + 1) * U * A
        else:
            Ein = E + Q_REL * np.abs(v) + Q_ABS * Bd
            y, Ey = conv_ref("fwd", v, wt, b, None, a_scale=Bd, E_a=Ein)
        raws.append((y, Ey))
        ymax = float(np.abs(y).max())
        out, Eo = bn_act64(y, Ey, gamma, beta, rm, rv, act, slope, pool)
        if i + 1 < len(st):
            Bd = eval_bound(ymax, None, None, gamma, beta, rm, rv, act, slope) if pool else eval_bound(true_max, wt, b, gamma, beta, rm, rv, act, slope)
            bds.append(Bd)
        v, E, true_max = out, Eo, float(np.abs(out).max())
    return v, E, bds, raws


# ---------------------------------------------------------------- CPU emulations of the P16 arithmetic (test_p16_paths_host.py)
def split_at(t, mag, n=2):
    """float32 torch tensor -> (n fp16 terms as float32, scale): scaled by the power of two that takes `mag` into [2^14, 2^15) (f16_scale_exp)"""
    s = 2.0 ** (14 - math.floor(math.log2(float(mag))))
    out, r = [], t * s
    for _ in range(n):
        h = r.half().float()
        out.append(h)
        r = r - h
    return out, s


EMULATIONS = {"p16": [(1, 0), (0, 1), (0, 0)], "without_x1w0": [(0, 1), (0, 0)], "without_x0w1": [(1, 0), (0, 0)], "single_term": [(0, 0)],
              "last_chunk_left_out": [(1, 0), (0, 1), (0, 0)]}


def emulate_conv(kind, op, a, b, shape, a_mag, b_mag):
    """One convolution as a P16 kernel computes it (float32 numpy in and out): op64's operands a, b split into two fp16 terms at the scale of
    a_mag / b_mag (an a-priori bound for an image, the tensor's own maximum for weights), the three products accumulated in fp32 (torch's
    float32 convolution of the term tensors), smallest first.  kind: a key of EMULATIONS; "last_chunk_left_out" drops the last 16 channels
    of the reduction (fwd: input channels, dgrad: output channels) or the last 64-pixel chunk (wgrad: the last image's last rows)."""
    import torch
    A, Bt = torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b))
    if kind == "last_chunk_left_out":
        A, Bt = A.clone(), Bt.clone()
        if op == "fwd":
            A[:, -16:] = 0
        elif op == "dgrad":
            A[:, -16:] = 0
        else:
            rows = max(64 // A.shape[3], 1)
            A[-1, :, -rows:] = 0
    (at, sa), (bt, sb) = split_at(A, a_mag), split_at(Bt, b_mag)
    y = None
    for i, j in EMULATIONS[kind]:
        p = cp.op64(op, at[i], bt[j], shape)
        y = p if y is None else y + p
    return (y / (sa * sb)).numpy()


def quantise_p16(v, Bd, terms=2):
    """float32 numpy -> the value a P16 image of scale magnitude Bd holds for it (the sum of its `terms` fp16 terms)"""
    import torch
    t, s = split_at(torch.from_numpy(np.ascontiguousarray(v, np.float32)), Bd, terms)
    return (sum(t) / s).numpy()


def emulate_eval32(c, x, params, bds, terms=2, slope=pp.LEAKY_SLOPE):
    """The evaluate() chain in float32 (torch float32 convolutions, post_paths' float32 activations) with every handed-over tensor quantised to a
    P16 image of `terms` fp16 terms at the scale of its Bd -> (out, [each stage's raw convolution output])"""
    import torch
    F = torch.nn.functional
    v, raws = x, []
    for i, ((cin, co, h, w_, act, pool), (wt, b, gamma, beta, rm, rv)) in enumerate(zip(c.stages(), params)):
        ch = lambda t: np.asarray(t, np.float32)[None, :, None, None]
        y = (F.conv2d(torch.from_numpy(np.array(v)), torch.from_numpy(np.array(wt)), padding=1) + torch.from_numpy(np.array(b))[None, :, None, None]).numpy()
        raws.append(y)
        invstd = (1.0 / np.sqrt(rv.astype(np.float64) + pp.EPS)).astype(np.float32)
        z = ((y - ch(rm)) * ch(invstd)) * ch(gamma) + ch(beta)
        a = pp._act32(act, z, np.float32(slope)).astype(np.float32)
        if pool:
            w = pp._windows(a)
            a = ((((np.float32(0) + w[..., 0]) + w[..., 1]) + w[..., 2]) + w[..., 3]) / np.float32(4)
        v = quantise_p16(a, bds[i], terms) if i < len(bds) else a
    return v, raws
