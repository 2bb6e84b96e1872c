"""GR_GROUPCONV3 on the f16 / bf16 MFMA (csrc/groupmfma.hip), restated: the support rule, net.hip's dispatch rule, the grids, tile and step
counts, split counts and LDS / workspace arithmetic of the three launches; a case table whose named feature predicates reach every loop
step and edge of them; a float64 reference with a per-element bound; float32 emulations of the split arithmetics in kernel order.

Used by tests/test_groupmfma_paths_host.py (CPU) and tests/test_gpu_groupmfma_paths.py (-m gpu).  Every case is a one-stage net
([UPSAMPLE2,] GROUPCONV3 from a bare descriptor list) with 16 planes per group on both sides.

THE BOUND, per element (conv_paths' form): |got - ref64| <= U (c A + [f16x3] C16 M) + U |extra|.  A = the operation on the operands'
absolute values; M = (max|a| of the element's own (image, group) tile) * op(1, |b|) + (max|b| of its tile / its group's weights) *
op(|a|, 1) - the kernels scale per tile, so a small image beside a large one keeps its own precision (a weight-gradient element sums
the per-image terms); extra = the bias (forward) or the accumulated result (weight gradient: gw += s rounds once more).
c: the forward and the data gradient sum K = 144 products (x 4 behind an up-sampling, where the data gradient adds a 2 x 2 block) in the
order of a 3x3 split convolution: conv_paths.C_MODE.  The weight gradient sums pixel runs per wave, the four waves, images and splits in
order: its c is measured on the CPU with the emulation below and fixed at twice the largest value, rounded up (generic_paths' convention;
test_constants_are_twice_the_measured prints and holds it)."""
import dataclasses
import functools
import math
import zlib

import numpy as np

import conv_paths as cp

U = cp.U
C16 = cp.C16
MODES = ("f16x3", "bf16x6")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- groupmfma.hip and net.hip, restated
GM_PLANES, GM_MAX_HW, GM_KSTEPS, GM_MAX_SPLITS = 16, 32, 5, 16
GM_RED_FLOATS = 4 * 9 * 256
DEFAULT_MIN_TILES = 512                        # groupmfma.hip g_group_mfma_min_tiles
LDS_LIMIT = 160 * 1024                         # bytes of LDS a gfx950 workgroup may take
FP32_LABELS = frozenset({"groupconv3_forward_kernel", "groupconv3_dgrad_kernel", "groupconv3_wgrad_kernel", "group_wgrad_reduce_kernel"})
MFMA_LABELS = frozenset({"groupconv3_mfma_forward_kernel", "groupconv3_mfma_dgrad_kernel", "groupconv3_mfma_wgrad_kernel", "group_wgrad_reduce_kernel"})
UNIVERSE = FP32_LABELS | MFMA_LABELS


def supported(Cin, Cout, G, H, W, up):
    """groupmfma.hip groupconv3_mfma_supported"""
    return (G >= 1 and Cin == GM_PLANES * G and Cout == GM_PLANES * G and 1 <= H <= GM_MAX_HW and 1 <= W <= GM_MAX_HW
            and (not up or (H % 2 == 0 and W % 2 == 0)))


def dispatch(mode, B, Cin, Cout, G, H, W, up, min_tiles=DEFAULT_MIN_TILES):
    """net.hip group_mfma: the labels one forward + backward (gradInput wanted) of the stage records"""
    mfma = mode != "f32" and supported(Cin, Cout, G, H, W, up) and B * G >= min_tiles
    return set(MFMA_LABELS if mfma else FP32_LABELS)


def nterm(mode):
    return 2 if mode == "f16x3" else 3


def conv_launch(B, G, H, W, up, dgrad, nt):
    """groupconv3_mfma_conv_kernel<NTERM, DGRAD>: grid (G, B); staged planes Hs x Ws, written planes Ho x Wo; 16-pixel tiles (behind an
    up-sampling the data gradient's tiles are 4 source pixels x 4), two per wave and round, four waves"""
    up_in, up_out = (up and not dgrad), (up and dgrad)
    Hs, Ws = (H // 2, W // 2) if up_in else (H, W)
    Ho, Wo = (H // 2, W // 2) if up_out else (H, W)
    cells = (H + 2) * (W + 2)
    tiles = cdiv(Ho * Wo, 4) if up_out else cdiv(H * W, 16)
    return dict(grid=(G, B), Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, cells=cells, lds=nt * cells * 32, tiles=tiles, rounds=cdiv(tiles, 8),
                stage_items=2 * Hs * Ws, vec=(not up_out) and (H * W) % 4 == 0, up_in=up_in, up_out=up_out)


def wgrad_launch(B, G, H, W, up, nt):
    """launch_groupconv3_mfma_backward_weight: grid (G, used); pitch P, 32-k steps, halves per LDS plane, LDS bytes, workspace floats"""
    splits = min(B, GM_MAX_SPLITS)
    per = cdiv(B, splits)
    used = cdiv(B, per)
    P = cp.round_up(W + 2, 8)
    ksteps = cdiv(H * P, 32)
    PL = ksteps * 32 + 2 * P + 16
    planes = nt * GM_PLANES * PL * 2
    return dict(grid=(G, used), splits=splits, per=per, used=used, last_images=B - (used - 1) * per, P=P, ksteps=ksteps, PL=PL,
                planes_bytes=planes, lds=max(planes, 4 * GM_RED_FLOATS), ws_floats=splits * GM_PLANES * G * GM_PLANES * 9,
                written=used * GM_PLANES * G * GM_PLANES * 9)


def workspace_floats(B, Cin, Cout, G):
    """group.hip groupconv3_workspace_bytes (without its 256 spare bytes), which net.hip sizes the workspace with"""
    return min(B, 16) * Cout * (Cin // G) * 9


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    B: int
    G: int
    H: int             # the convolution's planes (the net input is H/2 x W/2 when up)
    W: int
    up: bool = False
    amps: tuple = ()   # per-image amplitudes of x and gradOutput (default: all 1)

    @property
    def C(self):
        return GM_PLANES * self.G

    def descs(self):
        import ganrev._lib as L
        return ([(L.UPSAMPLE2, 0, 0, 0, 0.0, 0)] if self.up else []) + [(L.GROUPCONV3, self.C, self.C, self.G, 0.0, 0)]

    @property
    def dims(self):
        return (self.C, self.H // 2, self.W // 2) if self.up else (self.C, self.H, self.W)

    @property
    def in_shape(self):
        return (self.B,) + self.dims

    @property
    def out_shape(self):
        return (self.B, self.C, self.H, self.W)

    @property
    def n_weights(self):
        return self.C * GM_PLANES * 9

    def labels(self, mode, min_tiles):
        return dispatch(mode, self.B, self.C, self.C, self.G, self.H, self.W, self.up, min_tiles)

    def features(self):
        """named predicates of the three launches (the same for both arithmetics, but for the LDS sizes)"""
        B, G, H, W, up = self.B, self.G, self.H, self.W, self.up
        fw, dg, wg = conv_launch(B, G, H, W, up, False, 3), conv_launch(B, G, H, W, up, True, 3), wgrad_launch(B, G, H, W, up, 3)
        f = {}
        for tag, m in (("fwd", fw), ("dgrad", dg)):
            f[f"{tag} a wave takes a second round of tiles"] = m["rounds"] >= 2
            f[f"{tag} odd tile count: a round's second tile is past the end"] = m["tiles"] % 2 == 1
            f[f"{tag} waves without a tile"] = m["tiles"] <= 6
            f[f"{tag} staging loop: a partial round (some threads stage nothing)"] = m["stage_items"] % 256 != 0
            f[f"{tag} staging loop runs more than once"] = m["stage_items"] > 256
            f[f"{tag} border loop runs twice"] = m["cells"] > 256
        f["fwd ragged last 16-pixel tile"] = (H * W) % 16 != 0
        f["fwd a 16-pixel tile spans rows that are not aligned"] = W % 16 != 0 and H > 1
        f["fwd width exactly two pixel tiles"] = W == 32
        f["fwd 16-byte stores"] = fw["vec"]
        f["fwd scalar stores"] = not fw["vec"]
        f["fwd staged behind the up-sampling (four cells per source pixel)"] = fw["up_in"]
        f["fwd plain staging"] = not fw["up_in"]
        f["fwd 1x1 source: every tap but the centre block padded"] = fw["up_in"] and fw["Hs"] == 1 and fw["Ws"] == 1
        f["LDS at its largest (32 x 32)"] = H == GM_MAX_HW and W == GM_MAX_HW
        f["dgrad<up>: tiles of 4 source pixels x their 2 x 2 block"] = dg["up_out"]
        f["dgrad<up>: ragged last tile (source pixels % 4 != 0)"] = dg["up_out"] and (dg["Ho"] * dg["Wo"]) % 4 != 0
        f["dgrad plain with 16-byte stores"] = not dg["up_out"] and dg["vec"]
        f["dgrad plain with scalar stores"] = not dg["up_out"] and not dg["vec"]
        f["a second group's weights and planes"] = G >= 2
        f["G odd"] = G % 2 == 1
        f["wgrad per_split >= 2 and last split shorter"] = wg["per"] >= 2 and wg["last_images"] < wg["per"]
        f["wgrad used < splits"] = wg["used"] < wg["splits"]
        f["wgrad one image per split"] = wg["per"] == 1 and B >= 2
        f["wgrad a split walks several images (per-image scale-back, planes staged anew)"] = wg["per"] >= 2
        f["wgrad a wave takes a second k step"] = wg["ksteps"] >= 5
        f["wgrad a wave takes ten k steps"] = wg["ksteps"] >= 40
        f["wgrad waves without a k step"] = wg["ksteps"] < 4
        f["wgrad k tail beyond the plane (H P % 32 != 0)"] = (H * wg["P"]) % 32 != 0
        f["wgrad A fragment partly outside its row (W % 8 != 0)"] = W % 8 != 0
        f["wgrad A fragments wholly inside or outside (W % 8 == 0)"] = W % 8 == 0
        f["wgrad pitch 40 (W + 2 <= 40 < W + 8)"] = wg["P"] == 40
        f["wgrad pitch 8"] = wg["P"] == 8
        f["wgrad planes smaller than the cross-wave scratch"] = wg["planes_bytes"] < 4 * GM_RED_FLOATS
        f["wgrad planes larger than the cross-wave scratch"] = wg["planes_bytes"] > 4 * GM_RED_FLOATS
        f["wgrad staged behind the up-sampling"] = up
        f["wgrad plain staging"] = not up
        f["f16x3: a tile of zeros (scale 1)"] = 0.0 in self.amps
        f["f16x3: tiles 2^60 apart in one batch"] = bool(self.amps) and max(self.amps) / min(a for a in self.amps if a) >= 2.0 ** 60
        return f


# The issue's table, unchanged: every shape reaches the edge it is named for (test_every_required_feature_is_reached).
CASES = [
    Case("gm_mini", 3, 2, 8, 8, True),                     # G4's stage in small: 4 x 4 sources, 4 tiles, 4 + 4 dgrad tiles
    Case("gm_odd", 5, 3, 5, 7),                            # 35 pixels: 3 tiles (the last ragged, rows of 7 not aligned), scalar stores, pitch 16
    Case("gm_plane_max", 2, 1, 32, 32),                    # LDS at its largest, 64 tiles = 2 rounds per wave, 40 k steps
    Case("gm_g4_plane", 17, 2, 32, 32, True),              # G4's own plane; per 2, used 9 < 16 splits, the last split one image
    Case("gm_tiny", 1, 1, 2, 2, True),                     # 1 x 1 source; one ragged dgrad tile; 1 k step
    Case("gm_band", 2, 2, 3, 32),                          # width exactly two pixel tiles, three rows: 6 tiles, 4 k steps (3 x 40 = 120)
    Case("gm_zero_and_scales", 3, 1, 8, 8, True, (2.0 ** -30, 0.0, 2.0 ** 30)),
]
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(x, gout, w, b, params) float32, seeded by the case name, read-only.  x, gradOutput ~ N(0, 1) times the image's amplitude;
    weights U(-1, 1) / sqrt(144); biases U(-0.5, 0.5)"""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal(c.in_shape, dtype=np.float32)
    gout = rng.standard_normal(c.out_shape, dtype=np.float32)
    if c.amps:
        amp = np.array(c.amps, np.float32).reshape(-1, 1, 1, 1)
        x, gout = x * amp, gout * amp
    w = (rng.uniform(-1, 1, (c.C, GM_PLANES, 3, 3)) / 12.0).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, c.C).astype(np.float32)
    d = dict(x=x, gout=gout, w=w, b=b, params=np.concatenate([w.ravel(), b]))
    for v in d.values():
        v.setflags(write=False)
    return d


# ---------------------------------------------------------------- float64 reference and bound
# c of the weight gradient.  MEASURED on the CPU (emulate() against float64, largest err / (U A) over every case, the f16x3 term C16 M
# taken off first); C_WGRAD = twice that, rounded up: 8 and 3.  Both maxima come from gm_tiny, whose sums hold four products: in f16x3 the
# dropped x1 w1 and the low terms' rounding reach their 2^-22 |x||w| = 4 U per product with nothing to average against; the long sums of
# the 32 x 32 cases measure 0.3 - 1.
MEASURED_WGRAD = {"f16x3": 4.00, "bf16x6": 1.06}
C_WGRAD = {m: float(math.ceil(2 * v)) for m, v in MEASURED_WGRAD.items()}


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def down2(t):
    """sum of each 2 x 2 block (the up-sampling's backward)"""
    return t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2]


def _ops(c):
    """the three float64 operators of the case on torch tensors: fwd(x, w), dgrad(dy, w), wgrad(x, dy)"""
    import torch
    F = torch.nn.functional
    wshape = (c.C, GM_PLANES, 3, 3)
    up = (lambda t: cp.up2(t)) if c.up else (lambda t: t)
    dn = down2 if c.up else (lambda t: t)
    return (lambda x, w: F.conv2d(up(x), w, padding=1, groups=c.G),
            lambda dy, w: dn(F.conv_transpose2d(dy, w, padding=1, groups=c.G)),
            lambda x, dy: torch.nn.grad.conv2d_weight(up(x), wshape, dy, padding=1, groups=c.G))


def _tile_max(t, G):
    """max |.| of every (image, group) tile, broadcast back over the tile"""
    B, C = t.shape[:2]
    m = t.abs().reshape(B, G, -1).amax(2)
    return m.reshape(B, G, 1, 1, 1).expand(B, G, C // G, t.shape[2], t.shape[3]).reshape(t.shape)


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """{"out" | "gin" | "gw": (ref, bound, A)} float64, read-only, computed once per (case, arithmetic)"""
    import torch
    c, d = BY_NAME[name], inputs(name)
    X, Wt, D, bias = _t(d["x"]), _t(d["w"]), _t(d["gout"]), _t(d["b"])
    fwd, dgrad, wgrad = _ops(c)
    f16 = mode == "f16x3"
    cm = cp.C_MODE[mode]
    wmax = Wt.abs().reshape(c.G, -1).amax(1).reshape(c.G, 1, 1, 1, 1).expand(c.G, GM_PLANES, GM_PLANES, 3, 3).reshape(Wt.shape)
    out = {}
    A = fwd(X.abs(), Wt.abs())
    M = fwd(_tile_max(X, c.G), Wt.abs()) + fwd(X.abs(), wmax) if f16 else 0.0
    out["out"] = (fwd(X, Wt) + bias[None, :, None, None], U * (cm * A + C16 * M + bias.abs()[None, :, None, None]), A)
    A = dgrad(D.abs(), Wt.abs())
    M = dgrad(_tile_max(D, c.G), Wt.abs()) + dgrad(D.abs(), wmax) if f16 else 0.0
    out["gin"] = (dgrad(D, Wt), U * (cm * A + C16 * M), A)
    A = wgrad(X.abs(), D.abs())
    M = wgrad(_tile_max(X, c.G), D.abs()) + wgrad(X.abs(), _tile_max(D, c.G)) if f16 else 0.0
    ref = wgrad(X, D)
    out["gw"] = (ref, U * (C_WGRAD[mode] * A + C16 * M + ref.abs()), A)
    res = {}
    for k, (r, bnd, a) in out.items():
        res[k] = tuple(np.ascontiguousarray(v.numpy() if isinstance(v, torch.Tensor) else v) for v in (r, bnd, a))
        for v in res[k]:
            v.setflags(write=False)
    return res


def f16_slack(name, mode):
    """the C16 M part of the weight gradient's bound in units of U A, per element (test_constants_are_twice_the_measured takes it off)"""
    r, bnd, A = reference(name, mode)["gw"]
    return (bnd / U - np.abs(r) - C_WGRAD[mode] * A) / np.where(A > 0, A, 1.0)


def ratio(got, ref, bound):
    """|err| / bound per element; a zero bound (a tile of zeros without a bias) admits a zero error only"""
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


def check_bound(got, ref, bound, what):
    r = ratio(got, ref, bound)
    worst = np.unravel_index(int(np.argmax(r)), r.shape)
    g = np.asarray(got).reshape(ref.shape)
    assert np.all(r <= 1.0), (f"{what}: {int((r > 1.0).sum())} of {r.size} elements outside the bound; worst at {worst}: got {float(g[worst])!r}, "
                              f"float64 {ref[worst]!r}, bound {bound[worst]:.3e} (x{r[worst]:.1f})")
    return float(r[worst])


# ---------------------------------------------------------------- float32 emulations in kernel order (CPU)
EMULATIONS = {          # name -> (split, products kept as (A term, B term), smallest first, scale per "tile" or "tensor")
    "f16x3": ("f16", [(1, 0), (0, 1), (0, 0)], "tile"),
    "bf16x6": ("bf16", [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)], "tile"),
    "f16x3_without_x1w0": ("f16", [(0, 1), (0, 0)], "tile"),
    "bf16x6_without_order2": ("bf16", [(1, 0), (0, 1), (0, 0)], "tile"),
    "f16x3_scale_per_tensor": ("f16", [(1, 0), (0, 1), (0, 0)], "tensor"),
}


def _scale_exp(amax):
    """kernels.h f16_scale_exp on the float32 maximum: k with max * 2^k in [2^14, 2^15); 0 for a zero (or subnormal) maximum"""
    e = (np.asarray(amax, np.float32).view(np.uint32) >> 23) & 0xff
    return np.where(e == 0, 0, np.minimum(141 - e.astype(np.int64), 126))


def _terms(t, split, k):
    """t (float32 torch) -> the split's term tensors; f16: of t * 2^k (k broadcastable int array)"""
    import torch
    if split == "f16":
        r = t * torch.from_numpy(np.ldexp(np.float32(1), k).astype(np.float32))
        conv = lambda v: v.half().float()
        n = 2
    else:
        r, conv, n = t, (lambda v: v.to(torch.bfloat16).float()), 3
    out = []
    for _ in range(n):
        h = conv(r)
        out.append(h)
        r = r - h
    return out


def emulate(name, kind):
    """The case's forward, gradInput and weight gradient as float32 numpy: the operands split as the kernels split them (a power of two per
    (image, group) tile and per group's weights in f16x3), exact products of the terms, fp32 accumulation - per MFMA step (32 k) a float32
    dot, the steps and products chained in the kernels' order, then the waves, images and splits in order."""
    import torch
    F = torch.nn.functional
    c, d = BY_NAME[name], inputs(name)
    split, pairs, per = EMULATIONS[kind]
    B, G, C, H, W = c.B, c.G, c.C, c.H, c.W
    X, Wt, D, bias = (torch.from_numpy(np.array(d[k])) for k in ("x", "w", "gout", "b"))

    def tile_exp(t):                                   # [B][G] exponents, broadcast over the tensor
        m = t.abs().reshape(B, G, -1).amax(2).numpy()
        if per == "tensor":
            m = np.full_like(m, m.max())
        return _scale_exp(m)
    kx, kd = tile_exp(X), tile_exp(D)
    kw = _scale_exp(Wt.abs().reshape(G, -1).amax(1).numpy())
    if split != "f16":
        kx, kd, kw = kx * 0, kd * 0, kw * 0
    bc = lambda k, t: np.repeat(k, GM_PLANES, axis=1).reshape(B, C, 1, 1)          # [B][G] -> over t's channels
    xs = _terms(X, split, bc(kx, X))
    ds = _terms(D, split, bc(kd, D))
    ws = _terms(Wt, split, np.repeat(kw, GM_PLANES).reshape(C, 1, 1, 1))
    back = lambda acc, k: acc * torch.from_numpy(np.ldexp(np.float32(1), -k).astype(np.float32))
    if c.up:
        xs = [t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) for t in xs]
    # forward: k = 16 tap + plane, steps of two taps
    acc = torch.zeros(c.out_shape)
    for s in range(GM_KSTEPS):
        mask = torch.zeros(1, 1, 9)
        mask[..., 2 * s:2 * s + 2] = 1
        for i, j in pairs:
            acc = acc + F.conv2d(xs[i], ws[j] * mask.reshape(1, 1, 3, 3), padding=1, groups=G)
    out = back(acc, bc(kx, acc) + np.repeat(kw, GM_PLANES).reshape(1, C, 1, 1)) + bias[None, :, None, None]
    # data gradient: the same loop over the flipped taps 8 - tap
    acc = torch.zeros(c.out_shape)
    for s in range(GM_KSTEPS):
        mask = torch.zeros(1, 1, 9)
        for tap in (2 * s, 2 * s + 1):
            if tap < 9:
                mask[..., 8 - tap] = 1
        for i, j in pairs:
            acc = acc + F.conv_transpose2d(ds[i], ws[j] * mask.reshape(1, 1, 3, 3), padding=1, groups=G)
    if c.up:
        acc = ((acc[:, :, 0::2, 0::2] + acc[:, :, 0::2, 1::2]) + acc[:, :, 1::2, 0::2]) + acc[:, :, 1::2, 1::2]
    gin = back(acc, bc(kd, acc) + np.repeat(kw.reshape(1, G), GM_PLANES, axis=1).reshape(1, C, 1, 1))
    # weight gradient: k = y P + x; wave w takes steps w, w + 4, ...; waves, images, splits in order
    m = wgrad_launch(B, G, H, W, c.up, 2)
    P, ksteps = m["P"], m["ksteps"]
    K = ksteps * 32
    Gk = [F.pad(F.pad(t, (0, P - W)).reshape(B, G, GM_PLANES, H * P), (0, K - H * P)) for t in ds]                    # [B][G][oc][k]
    Xk = []
    for t in xs:
        tp = F.pad(t, (1, P - W + 1, 1, 1))                                                                              # rows H + 2, columns P + 2
        taps = torch.stack([tp[:, :, ky:ky + H, kx:kx + P] for ky in range(3) for kx in range(3)], dim=2)                # [B][C][9][H][P]
        Xk.append(F.pad(taps.reshape(B, G, GM_PLANES, 9, H * P), (0, K - H * P)).permute(0, 1, 3, 2, 4))                 # [B][G][9][ci][k]
    waves = []
    for wv in range(4):
        acc = torch.zeros(B, G, 9, GM_PLANES, GM_PLANES)                                                                # [tap][oc][ci]
        for step in range(wv, ksteps, 4):
            sl = slice(32 * step, 32 * step + 32)
            for i, j in pairs:
                acc = acc + torch.matmul(Gk[i][:, :, None, :, sl], Xk[j][..., sl].transpose(-1, -2))
        waves.append(acc)
    img = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    img = img * torch.from_numpy(np.ldexp(np.float32(1), -(kx + kd)).astype(np.float32)).reshape(B, G, 1, 1, 1)
    total = torch.zeros(G, 9, GM_PLANES, GM_PLANES)
    for sp in range(m["used"]):
        part = torch.zeros(G, 9, GM_PLANES, GM_PLANES)
        for bi in range(sp * m["per"], min(B, (sp + 1) * m["per"])):
            part = part + img[bi]
        total = total + part
    gw = total.permute(0, 2, 3, 1).reshape(C, GM_PLANES, 3, 3)                                                          # [g][oc][ci][tap]
    return dict(out=out.numpy(), gin=gin.numpy(), gw=gw.numpy())
