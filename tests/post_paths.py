"""The per-channel pipeline of csrc/elem.hip (BatchNorm statistics, BatchNorm apply, activation, Dropout / SpatialDropout, 2x2 max / average pool and
the two-pass backward) and the part of csrc/net.hip that routes a stage through it, restated; a case table; a float64 reference with a
per-element error bound; float32 emulations in the kernels' operation order.

Used by tests/test_post_paths_host.py (CPU: the table reaches every combination the mirror reaches on a grid, the hand-written expectations equal
the mirror, the inputs are conditioned, the bound accepts the emulation and rejects degraded ones) and tests/test_gpu_post_paths.py (every
observable of every case against the bound, the labels under the per-kernel timer against the mirror).

A stage is what net.hip plan_net makes of a run of layers: [main operator] [BatchNorm] [activation] [dropout] [pool] [dropout].  A PReLU closes
its stage; behind a BatchNorm it opens one.  Two kinds of nets:
  element-wise (ST_ELEM)  the net IS the stage: the pipeline's y is the net input, its dy is gradInput - both ends observed directly
  main-operator           3x3 convolution / Linear, then the pipeline: the reference takes the raw y from the device (layer_output of the
                          main layer); gradInput / gradWeight are compared with float64 gradients of the REFERENCE dy (conv_paths' bound for
                          the arithmetic plus the pipeline's bound on dy carried through |w| / |x|)

THE BOUND.  u = 2^-24 (one fp32 rounding: |fl(x) - x| <= u |x|).  First order in u; every bound is multiplied by SLACK = 1 + 2^-10 for the
products of two roundings.  Operation order as in the kernels (elem.hip compiles with -ffp-contract=off: every operation rounds):
  statistics  s = sum y, q = sum y^2 per channel.  Statistics pass (bn_stats_partial*_kernel + finalize): fp64 sums of the fp32 values; a
              thread, a block tree and the split loop are fewer than 2^12 additions in sequence: |ds| <= D sum|y|, |dq| <= D sum y^2,
              D = 2^-41.  Conv-epilogue tiles (conv3x3_fewin: pairwise sum of four, 6 wave-shuffle levels, in fp32; squares rounded once;
              then fp64): |ds| <= 8 u sum|y|, |dq| <= 9 u sum y^2.  m = s / n, vs = q - s m in fp64:
                E_mean64 = ds / n,  E_var = dq / n + 2 |m| ds / n
              mean32 = fl(m): E_mean = E_mean64 + u |m|.  invstd32 = fl(1 / sqrt(vs / n + eps)): relative r_inv = u + E_var / (2 (var + eps)).
              running: fl(0.1 m + 0.9 rm0) -> 0.1 E_mean64 + u |result|;  fl(0.1 vs / (n - 1) + 0.9 rv0) -> 0.1 E_var n / (n - 1) + u |result|
              evaluate(): mean32 = running mean (exact), invstd32 = fl(1 / sqrt(rv + eps)) in fp64: r_inv = u
  z           ((y - mean) * invstd) * g + bt, c = y - m:  fl(y - mean32): E_c = E_mean + u |c|;  * invstd32: + |c| (r_inv + u);  * g: + u;
              + bt: u |z|  =>  E_z = |g| invstd (E_mean + |c| (3 u + r_inv)) + u |z|
  activation  |act32(z32) - act(z)| <= L E_z + own:  ReLU L 1, exact.  LeakyReLU / PReLU L max(1, |slope|), one product: u |a|.
              Sigmoid L 1/4, Tanh L 1: C_ACT u |a| (expf / tanhf in float32 numpy against float64 on this module's pre-activations, doubled,
              as gemm_paths.C_ACT; test_post_paths_host.py re-measures).  ELU z <= 0: (v_exp_f32(z log2 e) - 1) * 1: the ELU_ABS = 3e-7 that
              elem.hip act_fwd documents, + u for the subtraction; z > 0 exact.
  masks       a * scale (scale = fl(1 / (1 - p)) taken as exact in the reference): + u |v| per mask; a dropped element is exactly 0
  max pool    the selected element's bound (the selection itself is the reference's: see CONDITIONING)
  avg pool    sum = 0; four fp32 additions in scan order (the first exact), / 4 exact: (sum E_v + 3 u sum|v|) / 4
  backward    g = ((gout * s2) [/ 4]) * s1: u |g| per mask.  dz = act'(z32) g:
                ELU z <= 0  g * ((e^z - 1) + 1): |g| (E_a + u) + u |dz|;  z > 0: E_g, + |g| E_z where z <= E_z (the derivative is continuous:
                            a branch taken the other way at z ~ 0 costs |g| |z|)    ReLU: E_g.    LeakyReLU / PReLU: L E_g + u |dz|
                Sigmoid     g * (1 - a) * a: |g| E_a + 3 u |dz|            Tanh  g * (1 - a * a): |g| (2 |a| E_a + u) + u |dz|
              without BatchNorm dy = dz.  Pass A: S = sum dz, Q = sum (y - mean32) * dz; the float4 kernels add four elements pairwise in fp32
              (two additions per element: 2 u) and round each product (u), the groups in fp64 (the scalar kernels: everything in fp64 - the
              same bound holds):  E_S = sum E_dz + 2 u sum|dz|;  E_Q = sum (|dz| E_c + |c| E_dz + 3 u |c dz|)
                gm = fl(S / n): E_S / n + u |gm|;   k = fl(Q invstd32^2 / n): E_Q invstd^2 / n + |k| (2 r_inv + u)
                ggamma = fl(Q invstd32): E_Q invstd + |ggamma| (r_inv + u);   gbeta = fl(S): E_S + u |gbeta|
              Pass B: dy = ((dz - gm) - (y - mean) * k) * invstd * w:
                t1 = dz - gm: E_dz + E_gm + u |t1|;  t2 = c k: |k| E_c + |c| E_k + u |t2|;  t3 = t1 - t2: + u |t3|;
                * invstd: invstd E_t3 + |t4| (r_inv + u);  * w: |w| E_t4 + u |dy|
              gbias = fl(sum dy) (pairwise four, then fp64): sum E_dy + 2 u sum|dy| + u |gbias| - with BatchNorm the true value is 0.
              PReLU slope: sum over z <= 0 of fl(gout * z) in fp64 (convk.hip prelu_grad_kernel): u sum|gout z| + u |result|

CONDITIONING.  Discrete decisions are the reference's alone: y is nudged on the CPU (and the statistics re-derived) until no ReLU / LeakyReLU /
PReLU input has |z| < MARGIN E_z and no max-pool window holds a value within MARGIN x its bound of the window's maximum without being equal to
it; MARGIN = 64.  Exact ties (masked zeros, zeroed planes, the gamma = 0 channel) stay: both sides resolve them in scan order.  No element is
excluded from any comparison, and pool_index() is compared byte for byte.  Main-operator stages take y from the device; the GPU test asserts
the same margins on that y."""
import dataclasses
import functools
import zlib

import numpy as np

import conv_paths as cp

U = 2.0 ** -24
D64 = 2.0 ** -41
SLACK = 1.0 + 2.0 ** -10
ELU_ABS = 3e-7
# expf / tanhf have no derivation in the project.  MEASURED, never with the kernel: float32 numpy against float64 on the fp32 pre-activations of
# this table's element-wise cases, largest |act32(z) - act64(z)| / (U |a|): Sigmoid 3.11, Tanh 1.81 (test_activation_constants_are_twice_the_measured
# prints them and holds the constants to it); twice that, rounded up to an integer.  (gemm_paths measured Sigmoid 2.59 on its narrower inputs.)
C_ACT = {"Sigmoid": 7.0, "Tanh": 4.0}
MARGIN = 64.0
EPS = 1e-5
LEAKY_SLOPE = 0.2
PRELU_SLOPE = 0.25
P_DROP, P_SDROP = 0.5, 0.25

# ---------------------------------------------------------------- the dispatch, restated
STAT_SPLITS, PB_SPLITS, T8_PXT = 64, 256, 1024          # kernels.h, elem.hip
F_SCALAR, F_VEC, F_G8 = "post_forward_kernel", "post_forward_vec_kernel", "post_forward_g8_kernel"
S_SCALAR, S_VEC, S_FIN, S_TILES = ("bn_stats_partial_kernel", "bn_stats_partial_vec_kernel", "bn_stats_finalize_kernel",
                                   "bn_stats_finalize_tiles_kernel")
A_SCALAR, A_VEC = "post_backward_a_kernel", "post_backward_a_vec_kernel"
B_SCALAR, B_VEC, B_G8 = "post_backward_b_kernel", "post_backward_b_vec_kernel", "post_backward_b_g8_kernel"
BIAS = "bias_grad_batch_kernel"
LABELS = frozenset({F_SCALAR, F_VEC, F_G8, S_SCALAR, S_VEC, S_FIN, S_TILES, A_SCALAR, A_VEC, B_SCALAR, B_VEC, B_G8, BIAS})
# (post_backward_finalize_kernel and bn_eval_prepare_kernel carry no KtScope: their cases are checked by value only)
ACTS = ("none", "ELU", "ReLU", "LeakyReLU", "Sigmoid", "Tanh", "PReLU")
KINK = ("ReLU", "LeakyReLU", "PReLU")


@dataclasses.dataclass(frozen=True)
class Stage:
    """net.hip post_args: what the pipeline kernels read from PostArgs.  m1 / m2: "none", "elem", "spatial" or "scale" (mask_ref)"""
    bn: bool = False
    act: str = "none"
    m1: str = "none"
    pool: str = "none"          # "none", "max", "avg"
    m2: str = "none"


def stage_of(layers, training):
    """net.hip plan_net + mask_ref for one stage's layers (after the main operator): "bn", an activation, "drop" (nn.Dropout(0.5), v2),
    "sdrop" (nn.SpatialDropout(0.25)), "max", "avg".  Dropout v2 is the identity in evaluate(), SpatialDropout a multiplication by 1 - p."""
    f = dict(bn=False, act="none", m1="none", pool="none", m2="none")
    phase = -1
    for l in layers:
        ph = 0 if l == "bn" else 1 if l in ACTS else 3 if l in ("max", "avg") else (4 if f["pool"] != "none" else 2)
        assert ph > phase and not (l == "PReLU" and f["bn"]), f"{layers}: not one stage"
        phase = ph
        if l == "bn":
            f["bn"] = True
        elif l in ACTS:
            f["act"] = l
        elif l in ("max", "avg"):
            f["pool"] = l
        else:
            kind = ("elem" if l == "drop" else "spatial") if training else ("none" if l == "drop" else "scale")
            f["m1" if ph == 2 else "m2"] = kind
    return Stage(**f)


def post_combo(f):
    """elem.hip post_combo: the compile-time specialisation (post_specialize<CB>) of the float4 and g8 kernels; 0 = generic"""
    if not f.bn and f.m2 == "none":
        if f.act == "PReLU" and f.m1 == "none" and f.pool == "none":
            return 4
        if f.act == "none" and f.m1 == "spatial" and f.pool == "max":
            return 5
        if f.act == "none" and f.m1 == "none" and f.pool == "max":
            return 6
        if f.act == "none" and f.m1 == "spatial" and f.pool == "none":
            return 7
        if f.act == "Sigmoid" and f.m1 == "none" and f.pool == "none":
            return 9
    if f.act == "ReLU" and f.bn and f.m1 == "none" and f.pool == "none" and f.m2 == "none":
        return 8
    if f.act != "ELU" or not f.bn:
        return 0
    if f.m1 == "elem" and f.pool == "none" and f.m2 == "none":
        return 1
    if f.m1 == "none" and f.pool == "max" and f.m2 == "elem":
        return 2
    if f.m1 == "spatial" and f.pool == "max" and f.m2 == "none":
        return 3
    if f.m1 == "none" and f.pool == "max" and f.m2 == "none":
        return 10
    if f.m1 == "scale" and f.pool == "max" and f.m2 == "none":
        return 11
    return 0


# elem.hip post_specialize<CB>, restated separately from post_combo: what each specialisation overwrites the stage description with.
# test_post_paths_host.py asserts post_combo(SPECIALIZED[cb]) == cb and that no other description maps to cb.
SPECIALIZED = {
    1: Stage(True, "ELU", "elem", "none", "none"), 2: Stage(True, "ELU", "none", "max", "elem"), 3: Stage(True, "ELU", "spatial", "max", "none"),
    4: Stage(False, "PReLU", "none", "none", "none"), 5: Stage(False, "none", "spatial", "max", "none"), 6: Stage(False, "none", "none", "max", "none"),
    7: Stage(False, "none", "spatial", "none", "none"), 8: Stage(True, "ReLU", "none", "none", "none"), 9: Stage(False, "Sigmoid", "none", "none", "none"),
    10: Stage(True, "ELU", "none", "max", "none"), 11: Stage(True, "ELU", "scale", "max", "none"),
}


def stat_splits(n):
    """elem.hip stat_splits"""
    return max(1, min(n // 4096, STAT_SPLITS))


def batch_splits(n, B):
    """elem.hip batch_splits: the float4 kernels slice the BATCH; re-derived from `per` so that every block owns an image (B = 29)"""
    s = min(stat_splits(n), B)
    per = -(-B // s)
    return -(-B // per)


def g8_slices(B):
    """elem.hip launch_post_backward: the operand-ready pass B slices the batch down to single images, up to PB_SPLITS slices"""
    s = min(B, PB_SPLITS)
    per = -(-B // s)
    return -(-B // per)


def post_g8_supported(C, H, W, pool, backward=False):
    """elem.hip post_g8_supported"""
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    if C % 8 or not ((W % 8 == 0 and H % 2 == 0) if pool else W % 4 == 0) or H * W < 64:
        return False
    n = H * W if backward else Ho * Wo
    return n % 256 == 0 and (n <= T8_PXT or n % T8_PXT == 0)


def g8_blocks(B, C, H, W, pool):
    """elem.hip launch_post_forward, the p16 branch: the grid; planes above 256 pixels take the `blocks *= 4` branch"""
    hwo = (H // 2) * (W // 2) if pool else H * W
    blocks = B * (C // 8) * (hwo // T8_PXT if hwo > T8_PXT else 1)
    if blocks > 4096 and hwo > 256:
        blocks = 4096
    if hwo > 256:
        blocks *= 4
    return min(blocks, 8192)


def post_big(B, C, H, W):
    """elem.hip post_big: non-temporal loads in pass A (and the g8 pass B) from 128 MB on"""
    return 4.0 * B * C * H * W >= 128.0 * 1024 * 1024


def fwd_vec(pool, B, C, H, W):
    """elem.hip launch_post_forward"""
    return ((W % 8 == 0 and H % 2 == 0) if pool else W % 4 == 0) and B * C * H * W < (1 << 32)


def stats_vec(HW):
    """elem.hip launch_bn_stats"""
    return HW % 4 == 0 and HW >= 64


def bwd_vec(pool, B, C, H, W):
    """elem.hip launch_post_backward: the forward's condition AND a plane of at least 64 elements"""
    return ((W % 8 == 0 and H % 2 == 0) if pool else W % 4 == 0) and H * W >= 64 and float(B * H * W) * C < 4.0e9


def conv_fewin_applies(Cin, W, up=False):
    """conv.hip conv_fewin_applies"""
    return Cin <= 3 and not up and W % 4 == 0 and W >= 4


def conv_stat_tiles(mode, B, Cin, Cout, H, W, in_p16=False):
    """Per-channel statistics tiles the forward convolution's epilogue leaves (net.hip fwd_conv3 -> stat_tiles_last; 0: the statistics pass
    runs).  Few-input kernels with Cout <= 256 (conv.hip launch_conv3x3_fewin: one tile per 32 x 32 block), the 512-pixel split kernels
    (launch_conv3x3_split_n; the leaf from conv_paths.split_leaf), the P16 kernels (in_p16: the count is not restated, only > 0)."""
    if conv_fewin_applies(Cin, W):
        return B * -(-W // 32) * -(-H // 32) if Cout <= 256 else 0
    m = cp.MODES[mode]
    if m == 0 or Cout <= 4:
        return 0
    if m == 2 and in_p16:
        return 1
    leaf = cp.split_leaf(2 if m == 2 else 3, B, Cout, H, W, False, 128)
    if leaf.startswith("conv3x3_split_wide_kernel<16"):
        return (B + 1) // 2
    if leaf.startswith("conv3x3_split_wide_kernel<32"):
        return B * -(-W // 32) * -(-H // 16)
    return 0


def stats_route(f, training, main, tiles):
    """net.hip fwd_post: "tiles" (bn_stats_finalize_tiles_kernel on what the conv epilogue left: stat_tiles_last > 0), "pass"
    (launch_bn_stats), "eval" (bn_eval_prepare_kernel, once), "none" (no BatchNorm)"""
    if not f.bn:
        return "none"
    if not training:
        return "eval"
    return "tiles" if main == "conv" and tiles > 0 else "pass"


@dataclasses.dataclass(frozen=True)
class Plan:
    combo: int
    fwd: str                 # F_*
    stats: str               # "none", "eval", "tiles", S_SCALAR, S_VEC
    nstat: int               # grid.y of the statistics pass (0: none)
    a: str                   # A_*, "" when the library refuses the backward (BatchNorm in evaluate() mode)
    na: int
    b: str                   # B_*, "" without BatchNorm / refused
    nb: int
    bias: bool               # a bias job is queued (main operator with BatchNorm)

    def brief(self):
        short = lambda s: {"": "-", "none": "none", "eval": "eval", "tiles": "tiles"}.get(s) or ("g8" if "g8" in s else "vec" if "vec" in s else "scalar")
        n = lambda k, c: f"{short(k)}/{c}" if c else short(k)
        return f"cb{self.combo} F:{short(self.fwd)} S:{n(self.stats, self.nstat)} A:{n(self.a, self.na)} B:{n(self.b, self.nb)}{' bias' if self.bias else ''}"

    def fwd_labels(self):
        out = {self.fwd: 1}
        if self.stats == "tiles":
            out[S_TILES] = 1
        elif self.stats in (S_SCALAR, S_VEC):
            out[self.stats] = 1
            out[S_FIN] = 1
        return out

    def bwd_labels(self):
        out = {}
        for k in (self.a, self.b):
            if k:
                out[k] = 1
        return out

    def key(self, f, main):
        """the combination the host test wants covered"""
        return (main, self.fwd, self.stats, self.a, self.b, self.combo, f.pool, f.m1, f.m2, f.bn)


def plan(f, training, B, C, H, W, main="elem", tiles=0, p16_out=False, dy_p16=False):
    """One stage through launch_post_forward / launch_bn_stats / launch_post_backward.  p16_out: net.hip fwd_post hands the next convolution its
    input operand-ready (pa.p16 set: needs post_g8_supported); dy_p16: backward_impl found a consumer for an operand-ready dy (p16_dy_ok)."""
    pool = f.pool != "none"
    n = B * H * W
    assert not p16_out or post_g8_supported(C, H, W, pool), "fwd_post: p16_out only where post_g8_supported"
    fwd = F_G8 if p16_out else F_VEC if fwd_vec(pool, B, C, H, W) else F_SCALAR
    route = stats_route(f, training, main, tiles)
    stats, nstat = route, 0
    if route == "pass":
        stats, nstat = (S_VEC, batch_splits(n, B)) if stats_vec(H * W) else (S_SCALAR, stat_splits(n))
    if f.bn and not training:
        return Plan(post_combo(f), fwd, stats, nstat, "", 0, "", 0, False)
    vec = bwd_vec(pool, B, C, H, W)
    a, na = (A_VEC, batch_splits(n, B)) if vec else (A_SCALAR, stat_splits(n))
    b, nb = "", 0
    if f.bn:
        assert not dy_p16 or post_g8_supported(C, H, W, pool, True)
        b, nb = (B_G8, g8_slices(B)) if vec and dy_p16 else (B_VEC, na) if vec else (B_SCALAR, na)
    return Plan(post_combo(f), fwd, stats, nstat, a, na, b, nb, f.bn and main != "elem")


def bias_launches(nstages_with_bias):
    """elem.hip launch_post_backward / net.hip backward_impl: the bias jobs of a backward are summed by one launch per 16 queued, and the rest at the end"""
    return -(-nstages_with_bias // 16)


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    B: int
    C: int
    H: int
    W: int
    layers: tuple            # the stage's layers behind the main operator
    expect: str              # Plan.brief(), written by hand from elem.hip / net.hip
    training: bool = True
    main: str = "elem"       # "elem", "conv" (3x3, cin -> C) or "linear" (cin -> C, H = W = 1)
    cin: int = 0
    depth: int = 1           # > 1: that many conv + stage repetitions (C -> C)

    @property
    def stage(self):
        return stage_of(self.layers, self.training)

    @property
    def tiles(self):
        return conv_stat_tiles("f32", self.B, self.cin, self.C, self.H, self.W) if self.main == "conv" else 0

    def plan(self):
        return plan(self.stage, self.training, self.B, self.C, self.H, self.W, self.main, self.tiles)

    @property
    def out_hw(self):
        return (self.H // 2, self.W // 2) if self.stage.pool != "none" else (self.H, self.W)


# The stage forms of the table: layers, training, and - by hand, from post_specialize's comments - the combo each must run on
FORMS = [
    ("cb1", ("bn", "ELU", "drop"), True, 1), ("cb2", ("bn", "ELU", "max", "drop"), True, 2), ("cb3", ("bn", "ELU", "sdrop", "max"), True, 3),
    ("cb4", ("PReLU",), True, 4), ("cb5", ("sdrop", "max"), True, 5), ("cb6", ("max",), True, 6), ("cb7", ("sdrop",), True, 7),
    ("cb8", ("bn", "ReLU"), True, 8), ("cb9", ("Sigmoid",), True, 9),
    ("cb10", ("bn", "ELU", "max", "drop"), False, 10), ("cb11", ("bn", "ELU", "sdrop", "max"), False, 11),
    # the generic kernel's distinct forms
    ("leaky", ("LeakyReLU",), True, 0), ("tanh", ("Tanh",), True, 0), ("bn_sigmoid", ("bn", "Sigmoid"), True, 0), ("bn_alone", ("bn",), True, 0),
    ("elu", ("ELU",), True, 0), ("drop_avg_drop", ("drop", "avg", "drop"), True, 0), ("bn_relu_avg", ("bn", "ReLU", "avg"), True, 0),
    ("both_masks", ("bn", "ELU", "drop", "max", "drop"), True, 0), ("bn_leaky_sdrop", ("bn", "LeakyReLU", "sdrop"), True, 0),
    ("bn_tanh_drop", ("bn", "Tanh", "drop"), True, 0),
    # evaluate(): running statistics, SpatialDropout as MASK_SCALE
    ("eval_sdrop", ("sdrop",), False, 0), ("eval_bn_tanh", ("bn", "Tanh"), False, 0), ("eval_bn_relu_sdrop_avg", ("bn", "ReLU", "sdrop", "avg"), False, 0),
]
# The four route combinations of an element-wise stage, by hand from the launchers (B = 3: one split everywhere):
#   9 x 7    W % 4 != 0, HW = 63 < 64: scalar everywhere; with a pool the odd last row and column are dropped (floor)
#   12 x 6   W % 4 != 0 but HW = 72 (% 4 == 0, >= 64): the float4 statistics kernel, everything else scalar
#   4 x 8    W % 8 == 0, HW = 32 < 64: forward float4, statistics and both backward passes scalar
#   6 x 16   W % 8 == 0, HW = 96: float4 everywhere; 24 float4 groups per plane (12 pooled): not a power of two, udivp divides
SHAPES = {(9, 7): ("scalar", "scalar", "scalar"), (12, 6): ("scalar", "vec", "scalar"), (4, 8): ("vec", "scalar", "scalar"), (6, 16): ("vec", "vec", "vec")}


def _sweep():
    out = []
    for i, (fname, layers, training, combo) in enumerate(FORMS):
        bn = "bn" in layers
        for j, ((H, W), (fw, st, bw)) in enumerate(SHAPES.items()):
            s = f"S:{st}/1" if bn and training else "S:eval" if bn else "S:none"
            a = "A:- B:-" if bn and not training else f"A:{bw}/1 B:{bw}/1" if bn else f"A:{bw}/1 B:-"
            out.append(Case(f"{fname}_{H}x{W}", 3, 5 + (i + j) % 3, H, W, layers, f"cb{combo} F:{fw} {s} {a}", training))
    return out


CASES = _sweep() + [
    # ---- splits
    Case("b29_21_to_15_slices", 29, 3, 48, 64, ("bn", "ELU", "drop"), "cb1 F:vec S:vec/15 A:vec/15 B:vec/15"),      # 29 images over min(21, 29) -> per 2 -> 15 slices of 1536 groups: a full prefetch round and half a one; the last slice one image
    Case("stat_splits_cap_b128", 128, 3, 64, 64, ("bn", "ReLU"), "cb8 F:vec S:vec/64 A:vec/64 B:vec/64"),           # n / 4096 = 128 -> STAT_SPLITS, two images (two whole rounds) per slice
    Case("three_rounds_last_partial", 5, 3, 40, 64, ("bn", "ELU", "max", "drop"), "cb2 F:vec S:vec/3 A:vec/3 B:vec/3"),   # n = 12800 -> 3 splits, per 2: 1280 groups = 1024 + 256; last slice one image of 640
    Case("slice_below_256_groups", 2, 7, 8, 8, ("bn", "ELU", "sdrop", "max"), "cb3 F:vec S:vec/1 A:vec/1 B:vec/1"),  # 32 groups in all
    Case("scalar_splits_3", 4, 3, 65, 63, ("bn", "Tanh", "drop"), "cb0 F:scalar S:scalar/3 A:scalar/3 B:scalar/3"),  # the scalar kernels' element chunks: n = 16380 -> 3 chunks that straddle images
    # ---- main operator + pipeline (f32 arithmetic: the few-input convolution is fp32 VALU in every mode)
    Case("conv_tiles_3", 3, 5, 16, 16, ("bn", "ELU", "drop"), "cb1 F:vec S:tiles A:vec/1 B:vec/1 bias", main="conv", cin=3),              # 3 tiles: the first trip, one lane column
    Case("conv_tiles_66", 66, 6, 8, 8, ("bn", "ELU", "drop"), "cb1 F:vec S:tiles A:vec/1 B:vec/1 bias", main="conv", cin=1),          # 66 tiles: a second 64-lane column
    Case("conv_tiles_520", 520, 7, 4, 4, ("bn", "ELU", "drop"), "cb1 F:vec S:tiles A:scalar/2 B:scalar/2 bias", main="conv", cin=2),   # 520 tiles: the second trip of the 512-wide loop
    Case("conv_pass_cin4", 3, 5, 8, 8, ("bn", "ELU", "drop"), "cb1 F:vec S:vec/1 A:vec/1 B:vec/1 bias", main="conv", cin=4),  # no few-input kernel: the statistics pass on a conv output
    Case("conv_sigmoid_no_bn", 3, 5, 8, 12, ("Sigmoid",), "cb9 F:vec S:none A:vec/1 B:-", main="conv", cin=3),                    # post_backward_finalize_kernel's bias path
    Case("conv_prelu_no_bn", 3, 6, 9, 7, ("PReLU",), "cb4 F:scalar S:none A:scalar/1 B:-", main="conv", cin=3),                   # ... from the scalar pass A, with the slope gradient
    # (the remaining routes of the three convolution stage forms: test_post_paths_host.py wants every one the mirror reaches on its grid)
    Case("conv_pass_9x7", 3, 6, 9, 7, ("bn", "ELU", "drop"), "cb1 F:scalar S:scalar/1 A:scalar/1 B:scalar/1 bias", main="conv", cin=4),
    Case("conv_pass_12x6", 3, 7, 12, 6, ("bn", "ELU", "drop"), "cb1 F:scalar S:vec/1 A:scalar/1 B:scalar/1 bias", main="conv", cin=4),
    Case("conv_pass_4x8", 3, 5, 4, 8, ("bn", "ELU", "drop"), "cb1 F:vec S:scalar/1 A:scalar/1 B:scalar/1 bias", main="conv", cin=4),
    Case("conv_sigmoid_9x7", 3, 6, 9, 7, ("Sigmoid",), "cb9 F:scalar S:none A:scalar/1 B:-", main="conv", cin=4),
    Case("conv_sigmoid_4x8", 3, 7, 4, 8, ("Sigmoid",), "cb9 F:vec S:none A:scalar/1 B:-", main="conv", cin=3),
    Case("conv_prelu_4x8", 3, 5, 4, 8, ("PReLU",), "cb4 F:vec S:none A:scalar/1 B:-", main="conv", cin=3),
    Case("conv_prelu_6x16", 3, 7, 6, 16, ("PReLU",), "cb4 F:vec S:none A:vec/1 B:-", main="conv", cin=4),
    Case("linear_bn1d_relu", 5, 37, 1, 1, ("bn", "ReLU"), "cb8 F:scalar S:scalar/1 A:scalar/1 B:scalar/1 bias", main="linear", cin=11),
    Case("chain_17_bias_jobs", 3, 4, 8, 8, ("bn",), "cb0 F:vec S:vec/1 A:vec/1 B:vec/1 bias", main="conv", cin=4, depth=17),      # the bias-job list flushes at 16: two launches
]
BY_NAME = {c.name: c for c in CASES}
# The non-temporal loads of passes A and B (launch_post_backward: a.nt = post_big): exactly at the 128 MB threshold.  An element-wise net; its
# reference is computed channel by channel (test_gpu_post_paths.py).  MEASURED on the CPU: inputs, conditioning and reference 12 s.
NT_CASE = Case("nt_post_big_threshold", 32, 64, 128, 128, ("bn", "ReLU"), "cb8 F:vec S:vec/32 A:vec/32 B:vec/32")


# ---------------------------------------------------------------- the operand-ready (g8) kernels: a producer stage in front of a P16 consumer
def conv_p16_supported(B, Cin, Cout, H, W, min_tiles):
    """conv.hip conv_p16_supported (min_tiles = g_p16_min_tiles: 128, the tests force 1)"""
    if Cin % 16 or (H * W) % 256 or cp.round_up(Cout, 32) % 64 or B * Cin * H * W * 4 >= 0x7FFFF000:
        return False
    otiles = cp.round_up(Cout, 32) // 64
    if H == 16 and W == 16:
        return (B + 1) // 2 * otiles >= min_tiles
    return W >= 32 and W % 32 == 0 and H % 16 == 0 and B * (H // 16) * (W // 32) * otiles >= min_tiles


def conv_wgrad_p16_supported(B, Cin, Cout, H, W):
    """conv.hip conv_wgrad_p16_supported"""
    return Cin % 64 == 0 and Cout % 64 == 0 and W in (16, 32, 64) and (H * W) % 256 == 0 and B * max(Cin, Cout) * H * W * 4 < 0x7FFFF000


G8_COUT = 64


@dataclasses.dataclass(frozen=True)
class G8Case:
    """f16x3 mode: conv(1 -> C1) + `layers` (the producer stage, BatchNorm first), then conv(C1 -> 64) + BatchNorm (the consumer).  seed: chosen
    on the CPU (float64 convolution of the input) so that no kink input / max-pool window of the producer lies within 2 MARGIN of a decision;
    the GPU test asserts MARGIN on the device's own y."""
    name: str
    B: int
    C1: int
    H: int
    W: int
    layers: tuple
    expect: tuple            # Plan.brief() of the producer and of the consumer at p16_min_tiles = 1, and "lean" / "kept"
    seed: int = 0
    full: bool = True        # False: the convolution gradients are compared between the runs only, not with float64 (B = 257: the reference's cost)

    @property
    def stage(self):
        return stage_of(self.layers, True)

    @property
    def out_hw(self):
        return (self.H // 2, self.W // 2) if self.stage.pool != "none" else (self.H, self.W)


def g8_plans(c, min_tiles=1, guarded=True):
    """net.hip forward_stages / fwd_post / backward_impl for a G8Case -> (producer Plan, consumer Plan, producer output operand-ready only).
    p16_input_ok, p16_dy_ok, p16_wgrad_ok, dgrad_p16 / wgrad_p16 and out_skipped, restated; kb_gen is current where the tile route ran."""
    f1, f2 = c.stage, Stage(bn=True)
    pool = f1.pool != "none"
    H2, W2 = c.out_hw
    p16_in2 = c.C1 % 16 == 0 and conv_p16_supported(c.B, c.C1, G8_COUT, H2, W2, min_tiles)                 # p16_input_ok(consumer)
    tiles1 = conv_stat_tiles("f16x3", c.B, 1, c.C1, c.H, c.W)
    p16_out1 = f1.bn and tiles1 > 0 and p16_in2 and post_g8_supported(c.C1, c.H, c.W, pool)
    tiles2 = conv_stat_tiles("f16x3", c.B, c.C1, G8_COUT, H2, W2, in_p16=p16_out1)
    dy_ok2 = tiles2 > 0 and post_g8_supported(G8_COUT, H2, W2, False, True)                                # kb_gen current and p16_dy_ok
    wgrad_ok2 = post_g8_supported(G8_COUT, H2, W2, False, True) and c.C1 % 16 == 0 and conv_wgrad_p16_supported(c.B, c.C1, G8_COUT, H2, W2)
    dgrad2 = dy_ok2 and conv_p16_supported(c.B, G8_COUT, c.C1, H2, W2, min_tiles)
    wgrad2 = dy_ok2 and p16_out1 and wgrad_ok2
    # the producer's own dy: its data gradient has one output plane and its input no operand-ready image - never operand-ready
    p1 = plan(f1, True, c.B, c.C1, c.H, c.W, "conv", tiles1, p16_out=p16_out1)
    p2 = plan(f2, True, c.B, G8_COUT, H2, W2, "conv", tiles2, dy_p16=dgrad2 or wgrad2)
    return p1, p2, (not guarded) and p16_out1 and wgrad_ok2


_G8 = "F:g8 S:tiles A:vec/1 B:vec/1 bias"
_C64 = "cb0 F:vec S:tiles A:vec/1 B:g8/"
G8_CASES = [
    G8Case("g8_16x16_cb1", 3, 64, 16, 16, ("bn", "ELU", "drop"), ("cb1 " + _G8, _C64 + "3 bias", "lean")),                     # 256-pixel planes, B odd
    G8Case("g8_max_from_32_cb2", 1, 64, 32, 32, ("bn", "ELU", "max", "drop"), ("cb2 " + _G8, _C64 + "1 bias", "lean"), seed=7),
    G8Case("g8_avg_from_32", 3, 64, 32, 32, ("bn", "Tanh", "avg"), ("cb0 " + _G8, _C64 + "3 bias", "lean")),
    G8Case("g8_32x32_four_tiles", 3, 64, 32, 32, ("bn", "Sigmoid"), ("cb0 " + _G8, _C64 + "3 bias", "lean")),                   # 1024 pixels: blocks *= 4
    G8Case("g8_64x64_cb1", 3, 64, 64, 64, ("bn", "ELU", "drop"), ("cb1 F:g8 S:tiles A:vec/3 B:vec/3 bias", "cb0 F:vec S:tiles A:vec/3 B:g8/3 bias", "lean")),   # 4096 pixels: four T8_PXT tiles per plane
    G8Case("g8_16x16_cb8_relu", 1, 64, 16, 16, ("bn", "ReLU"), ("cb8 " + _G8, _C64 + "1 bias", "lean")),
    G8Case("g8_c16_forward_only", 3, 16, 16, 16, ("bn", "Sigmoid"), ("cb0 " + _G8, "cb0 F:vec S:tiles A:vec/1 B:vec/1 bias", "kept")),   # 16 channels: no P16 gradient kernel takes the consumer's dy
    G8Case("g8_b257_two_images_per_slice", 257, 64, 16, 16, ("bn", "ELU", "drop"), ("cb1 F:g8 S:tiles A:vec/16 B:vec/16 bias", "cb0 F:vec S:tiles A:vec/16 B:g8/129 bias", "lean"), full=False),
]
G8_BY_NAME = {c.name: c for c in G8_CASES}


def g8_inputs(c):
    """x (B, 1, H, W), the two convolutions' weights and biases, the two stages' parameters / masks (stage_inputs with y left to the device)"""
    rng = _rng(f"{c.name} main {c.seed}")
    x = rng.standard_normal((c.B, 1, c.H, c.W), dtype=np.float32)
    w1 = (rng.uniform(-1, 1, (c.C1, 1, 3, 3)) / 3.0).astype(np.float32)
    b1 = rng.uniform(-0.5, 0.5, c.C1).astype(np.float32)
    w2 = (rng.uniform(-1, 1, (G8_COUT, c.C1, 3, 3)) / np.sqrt(9.0 * c.C1)).astype(np.float32)
    b2 = rng.uniform(-0.5, 0.5, G8_COUT).astype(np.float32)
    H2, W2 = c.out_hw
    z = lambda *s: np.zeros(s, np.float32)
    d1 = stage_inputs(f"{c.name} 1 {c.seed}", c.stage, True, c.B, c.C1, c.H, c.W, y=z(c.B, c.C1, c.H, c.W))
    d2 = stage_inputs(f"{c.name} 2 {c.seed}", Stage(bn=True), True, c.B, G8_COUT, H2, W2, y=z(c.B, G8_COUT, H2, W2))
    return x, w1, b1, w2, b2, d1, d2


def g8_seed_ok(c, margin=2 * MARGIN):
    """the producer's decisions on the float64 convolution of x: none within `margin` bounds (the device's y differs from it by ~1e-6 of the gap)"""
    x, w1, b1, _, _, d1, _ = g8_inputs(c)
    y = cp.op64("fwd", cp._t(x), cp._t(w1), w1.shape).numpy() + b1.astype(np.float64)[None, :, None, None]
    r = forward64(c.stage, True, dict(d1, y=y.astype(np.float32)), "tiles")
    kd, pg = conditioning(c.stage, r)
    return kd >= margin and pg >= margin


# ---------------------------------------------------------------- inputs
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def mask_scale(kind):
    """net.hip mask_ref, float32 arithmetic: Dropout v2 keeps x / (1 - p) in training; SpatialDropout keeps x, and multiplies by 1 - p in evaluate()"""
    if kind == "elem":
        return float(np.float32(1) / (np.float32(1) - np.float32(P_DROP)))
    if kind == "scale":
        return float(np.float32(1) - np.float32(P_SDROP))
    return 1.0


def stage_inputs(name, f, training, B, C, H, W, y=None):
    """Everything one stage needs, float32, seeded by `name`: y (unless given: a main operator's output), gamma (both signs, one exactly 0), beta,
    the running statistics the forward starts from, the dropout keep masks, the slope and gradOutput ~ 0.1 N(0, 1).  With a training-mode
    BatchNorm the channels of y sit 0 .. 32 spreads off zero: a statistic accumulated in fp32 misses the bound."""
    rng = _rng(name)
    spread = rng.uniform(0.5, 2.0, C)
    offset = (np.linspace(0.0, 32.0, C)[rng.permutation(C)] * spread) if f.bn else np.zeros(C)
    d = dict(spread=spread.astype(np.float32))
    if y is None:
        y = (offset[None, :, None, None] + spread[None, :, None, None] * rng.standard_normal((B, C, H, W))).astype(np.float32)
    d["y"] = y
    gamma = (rng.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 2, -1.0, 1.0)).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    if C > 1:
        gamma[C // 2] = 0.0
        gamma[-1] = -abs(gamma[-1])      # (C = 3: the odd index is the zeroed one)
        beta[C // 2] = 0.3               # the whole channel is the constant beta: away from the kink
    d["gamma"], d["beta"] = gamma, beta
    if training:
        d["rm0"], d["rv0"] = rng.uniform(-0.5, 0.5, C).astype(np.float32), rng.uniform(0.5, 2.0, C).astype(np.float32)
    else:                                # evaluate(): running statistics near the data's, not the identity
        d["rm0"] = (offset + spread * rng.uniform(-0.3, 0.3, C)).astype(np.float32)
        d["rv0"] = (spread ** 2 * rng.uniform(0.6, 1.6, C)).astype(np.float32)
    Ho, Wo = (H // 2, W // 2) if f.pool != "none" else (H, W)
    for key, kind, shape in (("keep1", f.m1, (B, C, H, W)), ("keep2", f.m2, (B, C, Ho, Wo))):
        if kind == "elem":
            d[key] = (rng.uniform(0, 1, shape) >= P_DROP).astype(np.uint8)
        elif kind == "spatial":
            k = (rng.uniform(0, 1, shape[:2]) >= P_SDROP).astype(np.uint8)
            k.flat[1] = 0                # at least one zeroed plane, at least one kept
            k.flat[0] = 1
            d[key] = k
    d["slope"] = np.float32(PRELU_SLOPE if f.act == "PReLU" else LEAKY_SLOPE)
    d["gout"] = (0.1 * rng.standard_normal((B, C, Ho, Wo))).astype(np.float32)
    return d


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The conditioned inputs of an element-wise case (cached: the tests share them and leave them unchanged) -> (d, nudged elements)"""
    c = BY_NAME[name]
    assert c.main == "elem"
    d = stage_inputs(name, c.stage, c.training, c.B, c.C, c.H, c.W)
    nudged = condition(c.stage, c.training, d)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d, nudged


# ---------------------------------------------------------------- float64 reference and bound
def _mask(f_kind, keep, shape):
    """the multiplier of a mask, float64, broadcast to `shape`"""
    s = mask_scale(f_kind)
    if f_kind == "elem":
        return keep.astype(np.float64) * s
    if f_kind == "spatial":
        return np.broadcast_to(keep.astype(np.float64)[:, :, None, None] * s, shape)
    return np.full(shape, s)


def _nmasks(f):
    return (f.m1 != "none") + (f.m2 != "none")


def act64(act, z, slope):
    if act == "ELU":
        return np.where(z <= 0, np.expm1(np.minimum(z, 0)), z)
    if act == "ReLU":
        return np.where(z > 0, z, 0.0)
    if act in ("LeakyReLU", "PReLU"):
        return np.where(z > 0, z, z * slope)
    if act == "Sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if act == "Tanh":
        return np.tanh(z)
    return z


def act_bound(act, z, a, Ez, slope):
    """bound of the activation's fp32 value given the bound of its input"""
    if act == "ELU":
        return np.where(z <= 0, Ez + ELU_ABS + U, Ez)
    if act in ("LeakyReLU", "PReLU"):
        return max(1.0, abs(slope)) * Ez + U * np.abs(a)
    if act == "Sigmoid":
        return 0.25 * Ez + C_ACT["Sigmoid"] * U * np.abs(a)
    if act == "Tanh":
        return Ez + C_ACT["Tanh"] * U * np.abs(a)
    return Ez            # ReLU, none: exact


def _windows(v):
    """(B, C, Ho, Wo, 4): the 2 x 2 windows in scan order (0,0) (0,1) (1,0) (1,1); an odd last row / column is dropped (floor, as THNN)"""
    B, C, H, W = v.shape
    Ho, Wo = H // 2, W // 2
    return v[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)


def _unwindows(w, H, W):
    """inverse of _windows; the dropped row / column gets 0"""
    B, C, Ho, Wo, _ = w.shape
    out = np.zeros((B, C, H, W), w.dtype)
    out[:, :, :2 * Ho, :2 * Wo] = w.reshape(B, C, Ho, Wo, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * Ho, 2 * Wo)
    return out


def forward64(f, training, d, route="pass"):
    """The stage's forward in float64 from the Torch7 definitions (nn.SpatialBatchNormalization with batch statistics, eps 1e-5, momentum 0.1
    and the unbiased running variance; the activation; nn.Dropout / nn.SpatialDropout; nn.SpatialMaxPooling / nn.SpatialAveragePooling(2,2,2,2))
    with every bound of the module docstring.  route: "pass" or "tiles" (how the device summed the statistics).  -> dict"""
    y = d["y"].astype(np.float64)
    B, C, H, W = y.shape
    n = B * H * W
    r = dict(n=n)
    ch = lambda t: np.asarray(t, np.float64)[None, :, None, None]
    slope = float(d["slope"])
    if f.bn:
        g, bt = d["gamma"].astype(np.float64), d["beta"].astype(np.float64)
        if training:
            m = y.mean((0, 2, 3))
            var = ((y - ch(m)) ** 2).mean((0, 2, 3))
            cs, cq = (8 * U, 9 * U) if route == "tiles" else (D64, D64)
            Em64 = cs * np.abs(y).mean((0, 2, 3))
            Evar = cq * (y * y).mean((0, 2, 3)) + 2 * np.abs(m) * Em64
            Em = Em64 + U * np.abs(m)
            rinv = U + Evar / (2 * (var + EPS))
            r["run_mean"] = 0.1 * m + 0.9 * d["rm0"].astype(np.float64)
            r["run_var"] = 0.1 * var * n / (n - 1) + 0.9 * d["rv0"].astype(np.float64)
            r["E_run_mean"] = SLACK * (0.1 * Em64 + U * np.abs(r["run_mean"]))
            r["E_run_var"] = SLACK * (0.1 * Evar * n / (n - 1) + U * np.abs(r["run_var"]))
        else:
            m, var = d["rm0"].astype(np.float64), d["rv0"].astype(np.float64)
            Em, rinv = np.zeros(C), np.full(C, U)
        invstd = 1.0 / np.sqrt(var + EPS)
        c = y - ch(m)
        z = c * ch(invstd) * ch(g) + ch(bt)
        Ec = ch(Em) + U * np.abs(c)
        Ez = np.abs(ch(g * invstd)) * (ch(Em) + np.abs(c) * (3 * U + ch(rinv))) + U * np.abs(z)
        r.update(mean=m, var=var, invstd=invstd, rinv=rinv, c=c, Ec=Ec, gamma=g)
    else:
        z, Ez = y, np.zeros_like(y)
    a = act64(f.act, z, slope)
    Ea = act_bound(f.act, z, a, Ez, slope)
    m1 = _mask(f.m1, d.get("keep1"), y.shape)
    v = a * m1
    Ev = np.where(m1 != 0, m1 * Ea + (U * np.abs(v) if f.m1 != "none" else 0.0), 0.0)
    r.update(z=z, Ez=Ez, a=a, Ea=Ea, m1=m1, v=v, Ev=Ev)
    if f.pool == "max":
        w, Ew = _windows(v), _windows(Ev)
        idx = np.argmax(w, -1)               # first maximum in scan order: "first strictly greater wins"
        o = np.take_along_axis(w, idx[..., None], -1)[..., 0]
        Eo = np.take_along_axis(Ew, idx[..., None], -1)[..., 0]
        r["idx"] = idx.astype(np.uint8)
    elif f.pool == "avg":
        w, Ew = _windows(v), _windows(Ev)
        o = w.sum(-1) / 4
        Eo = (Ew.sum(-1) + 3 * U * np.abs(w).sum(-1)) / 4
    else:
        o, Eo = v, Ev
    m2 = _mask(f.m2, d.get("keep2"), o.shape)
    out = o * m2
    r.update(m2=m2, out=out, E_out=SLACK * np.where(m2 != 0, m2 * Eo + (U * np.abs(out) if f.m2 != "none" else 0.0), 0.0))
    return r


def backward64(f, d, r, gout=None, Eg_in=None, bias=False):
    """The stage's backward in float64 (BatchNorm backward through the two means) from forward64's record, with the bounds.  gout / Eg_in: the
    gradient wrt the stage output and its own bound (a chain hands them down); default d["gout"], exact."""
    gout = d["gout"].astype(np.float64) if gout is None else gout
    Eg = np.zeros_like(gout) if Eg_in is None else Eg_in
    slope = float(d["slope"])
    z, a, Ez, Ea = r["z"], r["a"], r["Ez"], r["Ea"]
    B, C, H, W = z.shape
    n = r["n"]
    ch = lambda t: np.asarray(t, np.float64)[None, :, None, None]
    g = gout * r["m2"]
    Eg = Eg * r["m2"]
    if f.pool == "max":
        sel = (np.arange(4)[None, None, None, None, :] == r["idx"][..., None]).astype(np.float64)
        g, Eg = _unwindows(g[..., None] * sel, H, W), _unwindows(Eg[..., None] * sel, H, W)
    elif f.pool == "avg":
        g, Eg = _unwindows(np.repeat(g[..., None] / 4, 4, -1), H, W), _unwindows(np.repeat(Eg[..., None] / 4, 4, -1), H, W)
    g = g * r["m1"]
    Eg = Eg * r["m1"] + _nmasks(f) * U * np.abs(g)
    if f.act == "ELU":
        dz = np.where(z <= 0, g * np.exp(np.minimum(z, 0)), g)
        Edz = np.where(z <= 0, np.abs(g) * (Ea + U) + U * np.abs(dz) + Eg * np.exp(np.minimum(z, 0)), Eg + np.where(z > Ez, 0.0, np.abs(g) * Ez))
    elif f.act == "ReLU":
        dz, Edz = np.where(a > 0, g, 0.0), np.where(a > 0, Eg, 0.0)
    elif f.act in ("LeakyReLU", "PReLU"):
        dz = np.where(z > 0, g, g * slope)
        Edz = np.where(z > 0, Eg, abs(slope) * Eg + U * np.abs(dz))
    elif f.act == "Sigmoid":
        dz = g * (1 - a) * a
        Edz = np.abs(g) * Ea + 3 * U * np.abs(dz) + Eg * (1 - a) * a
    elif f.act == "Tanh":
        dz = g * (1 - a * a)
        Edz = np.abs(g) * (2 * np.abs(a) * Ea + U) + U * np.abs(dz) + Eg * (1 - a * a)
    else:
        dz, Edz = g, Eg
    b = dict(dz=dz)
    if f.act == "PReLU":
        prod = np.where(z <= 0, gout * z, 0.0)        # (a PReLU stage holds nothing behind the PReLU: gout is its gradOutput, z its input)
        b["gslope"] = prod.sum()
        b["E_gslope"] = SLACK * (U * np.abs(prod).sum() + U * abs(b["gslope"]) + (np.abs(z) * (Eg_in if Eg_in is not None else 0.0)).sum())
    sum_c = lambda t: t.sum((0, 2, 3))
    if f.bn:
        c, Ec, invstd, rinv, w = r["c"], r["Ec"], r["invstd"], r["rinv"], r["gamma"]
        S, Q = sum_c(dz), sum_c(c * dz)
        ES = sum_c(Edz) + 2 * U * sum_c(np.abs(dz))
        EQ = sum_c(np.abs(dz) * Ec + np.abs(c) * Edz + 3 * U * np.abs(c * dz))
        gm, k = S / n, Q * invstd ** 2 / n
        Egm = ES / n + U * np.abs(gm)
        Ek = EQ * invstd ** 2 / n + np.abs(k) * (2 * rinv + U)
        b["ggamma"], b["E_ggamma"] = Q * invstd, SLACK * (EQ * invstd + np.abs(Q * invstd) * (rinv + U))
        b["gbeta"], b["E_gbeta"] = S, SLACK * (ES + U * np.abs(S))
        t1 = dz - ch(gm)
        t2 = c * ch(k)
        t3 = t1 - t2
        Et3 = (Edz + ch(Egm) + U * np.abs(t1)) + (np.abs(ch(k)) * Ec + np.abs(c) * ch(Ek) + U * np.abs(t2)) + U * np.abs(t3)
        t4 = t3 * ch(invstd)
        Et4 = ch(invstd) * Et3 + np.abs(t4) * ch(rinv + U)
        dy = t4 * ch(w)
        Edy = np.abs(ch(w)) * Et4 + U * np.abs(dy)
    else:
        dy, Edy = dz, Edz
    b["dy"], b["E_dy"] = dy, SLACK * Edy
    if bias:
        b["gbias"] = sum_c(dy)
        b["E_gbias"] = SLACK * (sum_c(Edy) + 2 * U * sum_c(np.abs(dy)) + U * np.abs(b["gbias"]))
    return b


def violations(f, r):
    """(kink mask, pool-window mask over (B, C, Ho, Wo)) of the decisions a rounding could turn"""
    kink = np.zeros(r["z"].shape, bool)
    if f.act in KINK:
        kink = np.abs(r["z"]) < MARGIN * r["Ez"]
    pool = None
    if f.pool == "max":
        w, Ew = _windows(r["v"]), _windows(r["Ev"])
        top = w.max(-1, keepdims=True)
        Etop = np.take_along_axis(Ew, np.argmax(w, -1)[..., None], -1)
        pool = ((w != top) & (top - w < MARGIN * np.maximum(Ew, Etop))).any(-1)
    return kink, pool


def conditioning(f, r):
    """(min |z| / E_z over kink inputs, min gap / bound over max-pool windows' non-equal values): both must be >= MARGIN (inf: none)"""
    kd = np.inf
    if f.act in KINK and (r["Ez"] > 0).any():
        kd = float((np.abs(r["z"])[r["Ez"] > 0] / r["Ez"][r["Ez"] > 0]).min())
    pg = np.inf
    if f.pool == "max":
        w, Ew = _windows(r["v"]), _windows(r["Ev"])
        top = w.max(-1, keepdims=True)
        Etop = np.take_along_axis(Ew, np.argmax(w, -1)[..., None], -1)
        ne = w != top
        if ne.any():
            e = np.maximum(Ew, Etop)[ne]
            gaps = (top - w)[ne]
            pg = float((gaps[e > 0] / e[e > 0]).min()) if (e > 0).any() else np.inf
    return kd, pg


def condition(f, training, d, rounds=40):
    """Nudge y (in place; float32) away from every decision a rounding could turn, re-deriving the statistics each round -> elements moved"""
    y = d["y"]
    step = (d["spread"] * np.float32(2.0 ** -6))[None, :, None, None] * np.ones(y.shape, np.float32)
    direction = np.sign(d["gamma"].astype(np.float64))[None, :, None, None] * np.ones(y.shape) if f.bn else np.ones(y.shape)
    moved = 0
    for _ in range(rounds):
        r = forward64(f, training, d)
        kink, pool = violations(f, r)
        push = np.zeros(y.shape)
        push[kink] = (np.where(r["z"] >= 0, 1.0, -1.0) * direction)[kink]          # z away from 0
        if pool is not None and pool.any():
            B, C, H, W = y.shape
            top = np.arange(4)[None, None, None, None, :] == r["idx"][..., None]
            up = _unwindows((top & pool[..., None]).astype(np.float64), H, W)     # the window's maximum moves up
            push = np.where(up != 0, direction, push)
        if not push.any():
            return moved
        moved += int((push != 0).sum())
        y += (push * step).astype(np.float32)
    raise AssertionError("conditioning did not settle")


def observables(f, training, d, route="pass", bias=False):
    """({name: (float64 reference, bound)}, the byte-exact pool index or None, forward64's and backward64's records) of one stage"""
    r = forward64(f, training, d, route)
    obs = {"out": (r["out"], r["E_out"])}
    if f.bn and training:
        obs["run_mean"], obs["run_var"] = (r["run_mean"], r["E_run_mean"]), (r["run_var"], r["E_run_var"])
    b = None
    if not (f.bn and not training):
        b = backward64(f, d, r, bias=bias)
        obs["dy"] = (b["dy"], b["E_dy"])
        for k in ("ggamma", "gbeta", "gslope", "gbias"):
            if k in b:
                obs[k] = (np.asarray(b[k]), np.asarray(b["E_" + k]))
    return obs, r.get("idx"), r, b


def check(got, ref, bound, what):
    """Every element within its bound (an exact reference wants an exact result) -> max |err| / bound"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = err > bound
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {err.size} elements outside the bound; worst at {worst}: got {float(np.asarray(got)[worst])!r}, "
                           f"float64 {float(np.asarray(ref)[worst])!r}, bound {float(np.asarray(bound)[worst]):.3e} (x{float(ratio[worst]):.1f})")
    return float(ratio[worst])


def worst_ratio(got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(ratio))


# ---------------------------------------------------------------- float32 emulation in the kernels' operation order (host test)
F32 = np.float32


def _act32(act, z, slope):
    if act == "ELU":
        return np.where(z <= 0, (np.exp(np.minimum(z, F32(0))) - F32(1)) * F32(1), z).astype(F32)
    if act == "ReLU":
        return np.where(z > 0, z, F32(0))
    if act in ("LeakyReLU", "PReLU"):
        return np.where(z > 0, z, z * slope)
    if act == "Sigmoid":
        return (F32(1) / (F32(1) + np.exp(-z))).astype(F32)
    if act == "Tanh":
        return np.tanh(z).astype(F32)
    return z


def _seq_sum32(t):
    """per channel, a sequential fp32 accumulation over (B, H, W)"""
    B, C = t.shape[:2]
    flat = np.ascontiguousarray(t.transpose(1, 0, 2, 3)).reshape(C, -1).astype(F32)
    return np.cumsum(flat, axis=1, dtype=F32)[:, -1].astype(np.float64)


def _group_sum(t, vec):
    """per channel: four consecutive elements of a row pairwise in fp32, the groups in fp64 (float4 kernels); everything in fp64 (scalar)"""
    if vec:
        q = t.reshape(t.shape[:3] + (t.shape[3] // 4, 4))
        t = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    return t.astype(np.float64).sum((0, 2, 3))


def emulate(f, training, d, wrong=None, nslices=1):
    """The stage as the kernels compute it, float32 -> the observables by name (+ "idx").  wrong: one degradation -
    "mask_shift" (mask 1's bits, or mask 2's without a mask 1, one bit off), "drop_last_slice" (the last of nslices batch slices missing from the
    statistics), "fp32_stats", "biased_running_var", "no_eps", "avg_no_quarter" (average pool's backward without / 4), "no_k" (BatchNorm
    backward without the k term), "combo_neighbour" (combo 10 <-> 11: mask 1 = MASK_SCALE exchanged with MASK_NONE)"""
    y = d["y"]
    B, C, H, W = y.shape
    n = B * H * W
    ch = lambda t: np.asarray(t, F32)[None, :, None, None]
    slope = F32(d["slope"])
    out = {}
    vecA = bwd_vec(f.pool != "none", B, C, H, W)

    def mask32(kind, keep, shape, which):
        if wrong == "combo_neighbour" and which == 1:
            kind = {"scale": "none", "none": "scale"}.get(kind, kind)
        s = F32(mask_scale(kind))
        if kind in ("elem", "spatial"):
            if wrong == "mask_shift" and (which == 1 or f.m1 == "none"):
                keep = np.roll(keep.reshape(-1), 1).reshape(keep.shape)
            k = keep.astype(F32) * s
            return k if kind == "elem" else np.broadcast_to(k[:, :, None, None], shape)
        return np.full(shape, s, F32)

    if f.bn:
        g, bt = ch(d["gamma"]), ch(d["beta"])
        if training:
            ys = y
            if wrong == "drop_last_slice":
                per = -(-B // nslices)
                ys = y[:per * (nslices - 1)]
            if wrong == "fp32_stats":
                s, q = _seq_sum32(ys), _seq_sum32(ys * ys)
            else:
                s, q = ys.astype(np.float64).sum((0, 2, 3)), (ys.astype(np.float64) ** 2).sum((0, 2, 3))
            m = s / n
            vs = np.maximum(q - s * m, 0)
            mean, invstd = m.astype(F32), (1.0 / np.sqrt(vs / n + (0.0 if wrong == "no_eps" else EPS))).astype(F32)
            out["run_mean"] = (0.1 * m + 0.9 * d["rm0"].astype(np.float64)).astype(F32)
            out["run_var"] = (0.1 * (vs / (n if wrong == "biased_running_var" else n - 1)) + 0.9 * d["rv0"].astype(np.float64)).astype(F32)
        else:
            mean = d["rm0"]
            invstd = (1.0 / np.sqrt(d["rv0"].astype(np.float64) + (0.0 if wrong == "no_eps" else EPS))).astype(F32)
        z = ((y - ch(mean)) * ch(invstd)) * g + bt
    else:
        z = y
    a = _act32(f.act, z, slope)
    m1 = mask32(f.m1, d.get("keep1"), y.shape, 1)
    v = a * m1
    if f.pool == "max":
        w = _windows(v)
        idx = np.argmax(w, -1)
        o = np.take_along_axis(w, idx[..., None], -1)[..., 0]
        out["idx"] = idx.astype(np.uint8)
    elif f.pool == "avg":
        w = _windows(v)
        o = (((F32(0) + w[..., 0]) + w[..., 1]) + w[..., 2] + w[..., 3]) / F32(4)
    else:
        o = v
    m2 = mask32(f.m2, d.get("keep2"), o.shape, 2)
    out["out"] = o * m2
    if f.bn and not training:
        return out
    gout = d["gout"]
    gg = gout * m2
    if f.pool == "max":
        sel = (np.arange(4)[None, None, None, None, :] == idx[..., None]).astype(F32)
        gg = _unwindows(gg[..., None] * sel, H, W)
    elif f.pool == "avg":
        gg = _unwindows(np.repeat((gg if wrong == "avg_no_quarter" else gg / F32(4))[..., None], 4, -1), H, W)
    gg = gg * m1
    if f.act == "ELU":
        dz = np.where(z <= 0, gg * (a + F32(1)), gg)
    elif f.act == "ReLU":
        dz = np.where(a > 0, gg, F32(0))
    elif f.act in ("LeakyReLU", "PReLU"):
        dz = np.where(z > 0, gg, gg * slope)
    elif f.act == "Sigmoid":
        dz = gg * (F32(1) - a) * a
    elif f.act == "Tanh":
        dz = gg * (F32(1) - a * a)
    else:
        dz = gg
    dz = dz.astype(F32)
    if f.act == "PReLU":
        out["gslope"] = F32(np.where(z <= 0, gout * z, F32(0)).astype(np.float64).sum())
    if not f.bn:
        out["dy"] = dz
        return out
    cm = y - ch(mean)
    S, Q = _group_sum(dz, vecA), _group_sum(cm * dz, vecA)
    i64 = invstd.astype(np.float64)
    gm, k = (S / n).astype(F32), (Q * i64 * i64 / n).astype(F32)
    out["ggamma"], out["gbeta"] = (Q * i64).astype(F32), S.astype(F32)
    if wrong == "no_k":
        k = np.zeros_like(k)
    out["dy"] = ((dz - ch(gm)) - cm * ch(k)) * ch(invstd) * g
    return out
