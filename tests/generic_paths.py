"""The generic route - the pointwise convolution (csrc/conv1x1.hip), the grouped layer kinds behind create_G4 (csrc/group.hip) and the 5x5
weight gradient (csrc/convk.hip) - with its launch arithmetic restated; a case table that reaches every loop iteration and tile edge of
those launches; a float64 reference with a per-element error bound; float32 emulations of the kernels' summation orders.

Used by tests/test_generic_paths_host.py (CPU: every REQUIRED_FEATURES entry is reached, the mirror names only KtScope labels of the sources,
the restated split / workspace arithmetic is consistent, the bound accepts the emulations and rejects degraded ones, the constants are
twice what the emulations measure) and tests/test_gpu_generic_paths.py (every element of every case against the bound, the recorded labels
against the mirror, += accumulation, bit-identity under the timer and across the three GR_CONV_MODEs).

Every case is a one-stage net (or UPSAMPLE2 + one stage) built from a bare descriptor list: the stage's input is the net input, its output
the raw operator output (no BatchNorm, no activation: the pipeline copies y and dy unchanged and sums the bias gradient).

THE BOUND, per element: |got - ref64| <= U * (c * A + |extra|), U = 2^-24.  A = the same operation on the absolute values of the operands;
extra = the bias (forward outputs: added once, one rounding), the accumulated result (weight gradients: `gw += s` rounds once more), 0
for data gradients.  c: see C_FAMILY below - measured on the CPU, never fitted to what the GPU returns.  Bias gradients are plain sums from
the pipeline backward: post_paths' rule for a bias sum with an exact dy, SLACK * (2 U sum|dy| + U |gbias|).  Multi-slope PReLU follows
post_paths too: forward and backward are one product where x <= 0 (U |w x|, U |w g|; exact copies where x > 0: bound 0), the slope gradient
(fp32 products, fp64 sums, one rounding to fp32) U sum|g x| + U |result|; all times SLACK = 1 + 2^-10.  No element is excluded anywhere."""
import dataclasses
import functools
import zlib

import numpy as np

import conv_paths as cp

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
MODES = ("f32", "bf16x6", "f16x3")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- conv1x1.hip, restated
C1_NT, C1_KC = 128, 32                         # pixels per workgroup, reduction channels per LDS chunk
C1_MAX_WGS, C1_MAX_SPLITS = 1024, 512


def c1_gemm(N, HW, K, M):
    """c1_launch + conv1x1_kernel<MB, WK>: forward K = Cin, M = Cout; data gradient K = Cout, M = Cin (WK = false).  MB = 32-plane blocks per
    workgroup; gridDim.y > 1 only with MB = 4; vec = 16-byte staging (the stage buffers are 16-byte aligned: see DESIGN.md);
    kn_last = the k-pair-rounded length of the last chunk."""
    MB = 1 if M <= 32 else (2 if M <= 64 else 4)
    chunks = cdiv(K, C1_KC)
    return dict(MB=MB, grid_x=cdiv(N, C1_NT), grid_y=cdiv(M, 128) if MB == 4 else 1, vec=HW % 4 == 0, k_chunks=chunks,
                kn_last=min(C1_KC, (K - (chunks - 1) * C1_KC + 1) & ~1))


def c1_split_cap(Cin, Cout):
    """conv1x1.hip c1_split_cap"""
    tiles = cdiv(Cin, 64) * cdiv(Cout, 64)
    return max(1, min(C1_MAX_WGS // tiles, C1_MAX_SPLITS))


def c1_wgrad(N, HW, Cin, Cout):
    """launch_conv1x1_backward_weight + conv1x1_wgrad_reduce_kernel: want, klen, splits, 32-pixel chunks per split, the last split's
    pixels, the reduce kernel's unrolled 16-blocks and tail; ws_floats = conv1x1_workspace_bytes, written = what the launch writes."""
    cap = c1_split_cap(Cin, Cout)
    want = min(cdiv(N, 32), cap)
    klen = cp.round_up(cdiv(N, want), 32)
    splits = cdiv(N, klen)
    last = N - (splits - 1) * klen
    return dict(cap=cap, want=want, klen=klen, splits=splits, chunks=klen // 32, last_pixels=last, last_chunks=cdiv(last, 32),
                in_tiles=cdiv(Cin, 64), out_tiles=cdiv(Cout, 64), vec=HW % 4 == 0, reduce16=splits // 16, reduce_tail=splits % 16,
                ws_floats=cap * Cin * Cout, written=splits * Cin * Cout)


# ---------------------------------------------------------------- group.hip, restated
GL_BT, GL_DB, GL_KC = 8, 4, 16
GC_OC, GC_CI, GC_WO, GC_MAX_SPLITS = 16, 8, 8, 16
PM_PARTS, PM_MAX_BLOCKS = 64, 4096


def gl_launch(B, a, b, G):
    """launch_grouplinear_forward / _backward_data / _backward_weight: grids and chunk counts"""
    Kg, Mg = a // G, b // G
    return dict(Kg=Kg, Mg=Mg, fwd_grid=(cdiv(b, 256), cdiv(B, GL_BT)), dgrad_grid=(G, cdiv(B, GL_DB)), wgrad_grid=cdiv(b, 256),
                k_chunks=cdiv(Kg, GL_KC), k_tail=Kg % GL_KC, m_rounds=cdiv(Mg, 256),
                block_sums=cdiv(Kg, GL_KC) * GL_DB * GL_KC)          # block_sum_256 calls of one dgrad workgroup, all on the same sh[4]


def gc_splits(B):
    """group.hip gc_splits"""
    return min(B, GC_MAX_SPLITS)


def gc_launch(B, Cin, Cout, G, H, W, up):
    """launch_groupconv3_forward / _backward_data / _backward_weight (H x W: the convolution's planes)"""
    Cg, Og, hw = Cin // G, Cout // G, H * W
    hwi = (H // 2) * (W // 2) if up else hw
    splits = gc_splits(B)
    per = cdiv(B, splits)
    used = cdiv(B, per)
    return dict(Cg=Cg, Og=Og, fwd_grid=(cdiv(hw, 256), G, B), oc_chunks=cdiv(Og, GC_OC), oc_tail=Og % GC_OC,
                dgrad_grid=(cdiv(hwi, 256), G, B), ci_chunks=cdiv(Cg, GC_CI), ci_tail=Cg % GC_CI,
                wgrad_grid=(Cin, cdiv(Og, GC_WO), used), wo_chunks=cdiv(Og, GC_WO), wo_tail=Og % GC_WO, pixel_rounds=cdiv(hw, 256),
                splits=splits, per=per, used=used, last_images=B - (used - 1) * per,
                ws_floats=splits * Cout * Cg * 9, written=used * Cout * Cg * 9)


def pm_blocks(n):
    """group.hip pm_blocks: workgroups of the multi-slope forward / backward kernels (256 threads, grid-stride)"""
    return max(1, min(cdiv(n, 1024), PM_MAX_BLOCKS))


def pm_launch(B, C, HW, ns):
    """launch_prelu_multi_forward / _backward / _grad: L elements per (sample, slope); parts partial sums per slope, laid out [slope][part]"""
    L = (C // ns) * HW
    total = B * L
    parts = max(1, min(cdiv(total, 1024), PM_PARTS))
    return dict(n=B * C * HW, blocks=pm_blocks(B * C * HW), blocks_wanted=cdiv(B * C * HW, 1024), L=L, total=total, parts=parts,
                parts_wanted=cdiv(total, 1024), grid_stride=total > parts * 256, ws_doubles=ns * PM_PARTS, written=ns * parts)


# ---------------------------------------------------------------- convk.hip (5x5 weight gradient), restated
KW_CI, KW_CO, KW_ROWS, KC_TILE = 16, 64, 8, 16
CONVK_MAX_SPLITS = 64


def convk_splits(B):
    """convk.hip convk_splits"""
    return min(B, CONVK_MAX_SPLITS)


def convk_image_floats(cin_eff, cout_eff, K):
    """convk.hip convk_image_floats (KC_CI * KC_KS = 32)"""
    return cp.round_up(cin_eff, 32) * K * K * cp.round_up(cout_eff, 32)


def k5_wgrad(B, Cin, Cout, H, W):
    """launch_convk_backward_weight, K = 5: grid (16-plane input blocks, 64-plane output blocks, splits); split z takes images z, z + splits, ..."""
    splits = convk_splits(B)
    return dict(splits=splits, grid=(cdiv(Cin, KW_CI), cdiv(Cout, KW_CO), splits), two_image_splits=max(0, B - splits) if B <= 2 * splits else splits,
                max_images=cdiv(B, splits), tiles=(cdiv(W, KC_TILE), cdiv(H, KW_ROWS)),
                ws_floats=max(convk_image_floats(Cin, Cout, 5), convk_image_floats(Cout, Cin, 5), splits * Cin * Cout * 25),
                written=splits * Cin * Cout * 25)


# ---------------------------------------------------------------- labels (KtScope names as they appear in the sources)
C1_LABELS = frozenset({"conv1x1_kernel", "conv1x1_kernel(dgrad)", "conv1x1_wgrad_kernel", "conv1x1_wgrad_reduce_kernel"})
GL_LABELS = frozenset({"grouplinear_forward_kernel", "grouplinear_dgrad_kernel", "grouplinear_wgrad_kernel"})
GC_LABELS = frozenset({"groupconv3_forward_kernel", "groupconv3_dgrad_kernel", "groupconv3_wgrad_kernel", "group_wgrad_reduce_kernel"})
PM_LABELS = frozenset({"prelu_multi_forward_kernel", "prelu_multi_backward_kernel", "prelu_multi_grad_kernel"})
K5_FIXED = frozenset({"convk_weight_image_kernel", "convk_wgrad_kernel", "convk_wgrad_reduce_kernel"})
K5_DIRECT = frozenset(cp.convk_direct_leaf(B, 32, 16, 16, bwd) for B in (1, 1024) for bwd in (False, True))
# every KtScope name of the three files; prelu_grad_kernel (convk.hip: the one-slope PReLU) is launched by none of these cases
UNIVERSE = C1_LABELS | GL_LABELS | GC_LABELS | PM_LABELS | K5_FIXED | K5_DIRECT | {"prelu_grad_kernel"}
SOURCES = ("conv1x1.hip", "group.hip", "convk.hip")


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str          # "c1" (CONVK c = 1), "gl" (GROUPLINEAR), "gc" (GROUPCONV3), "pm" (PRELU n >= 2), "k5" (CONVK c = 5)
    B: int
    Cin: int           # gl: a;  pm: C
    Cout: int          # gl: b;  pm: C
    H: int = 1         # the operator's planes (the net input is H/2 x W/2 when up)
    W: int = 1
    G: int = 1         # groups;  pm: the number of slopes
    up: bool = False

    def descs(self):
        import ganrev._lib as L
        if self.kind in ("c1", "k5"):
            return [(L.CONVK, self.Cin, self.Cout, 1 if self.kind == "c1" else 5, 0.0, 0)]
        if self.kind == "gl":
            return [(L.GROUPLINEAR, self.Cin, self.Cout, self.G, 0.0, 0)]
        if self.kind == "gc":
            return ([(L.UPSAMPLE2, 0, 0, 0, 0.0, 0)] if self.up else []) + [(L.GROUPCONV3, self.Cin, self.Cout, self.G, 0.0, 0)]
        return [(L.PRELU, self.G, 0, 0, 0.0, 0)]

    @property
    def dims(self):
        return (self.Cin, self.H // 2, self.W // 2) if self.up else (self.Cin, self.H, self.W)

    @property
    def in_shape(self):
        return (self.B, self.Cin) if self.kind == "gl" else (self.B,) + self.dims

    @property
    def out_shape(self):
        return (self.B, self.Cout) if self.kind == "gl" else (self.B, self.Cout, self.H, self.W)

    @property
    def modes(self):
        """the 1x1 and grouped kernels are exact fp32 in every GR_CONV_MODE; the 5x5 forward takes another kernel in f16x3"""
        return ("f32",) if self.kind == "k5" else MODES

    @property
    def n_weights(self):
        k = {"c1": 1, "k5": 25, "gc": 9, "gl": 1}.get(self.kind, 0)
        return self.Cout * (self.Cin // self.G) * k if self.kind != "pm" else 0

    def labels(self):
        """the labels of UNIVERSE one forward + backward (gradInput wanted) records"""
        if self.kind == "k5":
            return set(K5_FIXED) | {cp.convk_direct_leaf(self.B, self.Cout, self.H, self.W, False), cp.convk_direct_leaf(self.B, self.Cin, self.H, self.W, True)}
        return set({"c1": C1_LABELS, "gl": GL_LABELS, "gc": GC_LABELS, "pm": PM_LABELS}[self.kind])

    def features(self):
        """named predicates of the launches: what proves coverage (the 1x1 labels encode neither MB nor vec)"""
        B, HW = self.B, self.H * self.W
        N = B * HW
        f = {}
        if self.kind == "c1":
            fw, dg, wg = c1_gemm(N, HW, self.Cin, self.Cout), c1_gemm(N, HW, self.Cout, self.Cin), c1_wgrad(N, HW, self.Cin, self.Cout)
            for tag, m, K, M in (("fwd", fw, self.Cin, self.Cout), ("dgrad", dg, self.Cout, self.Cin)):
                f[f"c1_{tag}_MB == {m['MB']}"] = True
                f[f"c1_{tag}_MB == 4 and grid_y >= 2"] = m["MB"] == 4 and m["grid_y"] >= 2
                f[f"c1_{tag}_MB == 4 and the last block holds one plane"] = m["MB"] == 4 and M % 128 == 1
                f[f"c1_{tag}_k_chunks >= 3 with an odd tail (kn < 32)"] = m["k_chunks"] >= 3 and K % 2 == 1 and m["kn_last"] < 32
                f[f"c1_{tag}_k_chunks >= 2 with an even tail"] = m["k_chunks"] >= 2 and K % 2 == 0 and 0 < m["kn_last"] < 32
                f[f"c1_{tag}_K odd and below one chunk"] = K < C1_KC and K % 2 == 1
            f["c1_vec staging"] = fw["vec"]
            f["c1_scalar staging"] = not fw["vec"]
            f["c1_vec staging with HW below a tile"] = fw["vec"] and HW < C1_NT
            f["c1_pixel tile crosses an image boundary"] = B > 1 and HW % C1_NT != 0
            f["c1_ragged last pixel tile"] = N % C1_NT != 0
            f["c1_scalar staging and MB == 1"] = not fw["vec"] and fw["MB"] == 1 and dg["MB"] == 1
            f["c1_wgrad_chunks_per_split == 1"] = wg["chunks"] == 1
            f["c1_wgrad_chunks_per_split >= 2"] = wg["chunks"] >= 2
            f["c1_wgrad_chunks_per_split >= 3"] = wg["chunks"] >= 3
            f["c1_wgrad ragged last chunk inside a multi-chunk split"] = wg["last_chunks"] >= 2 and wg["last_pixels"] % 32 != 0
            f["c1_wgrad last split shorter: one ragged chunk behind multi-chunk splits"] = wg["chunks"] >= 2 and wg["last_chunks"] == 1 and wg["last_pixels"] % 32 != 0
            f["c1_wgrad last split ragged with single-chunk splits"] = wg["chunks"] == 1 and wg["last_pixels"] % 32 != 0
            f["c1_wgrad multi-chunk with vec tile loads"] = wg["chunks"] >= 2 and wg["vec"]
            f["c1_wgrad multi-chunk with scalar tile loads"] = wg["chunks"] >= 2 and not wg["vec"]
            f["c1_wgrad split count capped by c1_split_cap"] = cdiv(N, 32) > wg["cap"]
            f["c1_wgrad input-axis tiles >= 2"] = wg["in_tiles"] >= 2
            f["c1_wgrad output-axis tiles >= 2"] = wg["out_tiles"] >= 2
            f["c1_wgrad ragged channel tiles on both axes"] = self.Cin % 64 != 0 and self.Cout % 64 != 0
            f["c1_reduce 16-block and tail"] = wg["reduce16"] >= 1 and wg["reduce_tail"] >= 1
            f["c1_reduce tail only"] = wg["reduce16"] == 0
        elif self.kind == "gl":
            m = gl_launch(B, self.Cin, self.Cout, self.G)
            f["gl_fwd batch tiles >= 2 with a ragged last (GL_BT)"] = m["fwd_grid"][1] >= 2 and B % GL_BT != 0
            f["gl_fwd an output block of 256 holds a group boundary"] = any(o // m["Mg"] != min(o + 255, self.Cout - 1) // m["Mg"] for o in range(0, self.Cout, 256))
            f["gl_dgrad batch tiles >= 2 with a ragged last (GL_DB)"] = m["dgrad_grid"][1] >= 2 and B % GL_DB != 0
            f["gl_k_chunks >= 2 with a ragged last"] = m["k_chunks"] >= 2 and m["k_tail"] != 0
            f["gl_k exactly one full chunk"] = m["Kg"] == GL_KC
            f["gl_dgrad a second block_sum_256 round on reused sh"] = m["k_chunks"] >= 2
            f["gl_dgrad thread stride over Mg above 256"] = m["m_rounds"] >= 2
            f["gl_dgrad Mg below 256"] = m["Mg"] < 256
        elif self.kind == "gc":
            m = gc_launch(B, self.Cin, self.Cout, self.G, self.H, self.W, self.up)
            f["gc_fwd ragged second GC_OC chunk"] = m["oc_chunks"] >= 2 and m["oc_tail"] != 0
            f["gc_fwd pixel tiles >= 2"] = m["fwd_grid"][0] >= 2
            f["gc odd width"] = self.W % 2 == 1
            f["gc_dgrad ragged second GC_CI chunk"] = m["ci_chunks"] >= 2 and m["ci_tail"] != 0
            f["gc_wgrad ragged GC_WO chunks (>= 2)"] = m["wo_chunks"] >= 2 and m["wo_tail"] != 0
            f["gc_wgrad thread loop over pixels runs twice"] = m["pixel_rounds"] >= 2
            f["gc_per_split >= 2 and last split shorter"] = m["per"] >= 2 and m["last_images"] < m["per"]
            f["gc used < splits"] = m["used"] < m["splits"]
            f["gc_dgrad<1> (up-sampled) with input-pixel tiles >= 2"] = self.up and m["dgrad_grid"][0] >= 2
            f["gc_dgrad<0>"] = not self.up
        elif self.kind == "pm":
            m = pm_launch(B, self.Cin, HW, self.G)
            f["pm 1 < parts < PM_PARTS"] = 1 < m["parts"] < PM_PARTS and m["parts_wanted"] == m["parts"]
            f["pm parts capped at PM_PARTS with the grid-stride loop"] = m["parts_wanted"] > PM_PARTS and m["grid_stride"]
            f["pm_blocks capped at 4096"] = m["blocks_wanted"] > PM_MAX_BLOCKS
            f["pm L not a multiple of 256"] = m["L"] % 256 != 0
        else:
            m = k5_wgrad(B, self.Cin, self.Cout, self.H, self.W)
            f["k5_wgrad image loop steps (b += gridDim.z) in some splits only"] = 0 < m["two_image_splits"] < m["splits"]
            f["k5_wgrad blockIdx.y >= 1 with a ragged tail"] = m["grid"][1] >= 2 and self.Cout % KW_CO != 0
            f["k5_wgrad blockIdx.x >= 1 with a ragged tail"] = m["grid"][0] >= 2 and self.Cin % KW_CI != 0
            f["k5_wgrad ragged 8x16 tiles on both axes"] = self.H % KW_ROWS != 0 and self.W % KC_TILE != 0 and min(m["tiles"]) >= 2
        return f


# The smallest shapes that reach the edges (N = B * H * W).  One shape differs from the issue's table: c1_scalar_small is 6x9, not 6x10 - at
# HW = 60 (% 4 == 0) the mirror says the staging is the 16-byte one, and "scalar staging with MB == 1" would be lost; 6x9 (HW 54) keeps it.
CASES = [
    Case("c1_scalar_small", "c1", 3, 5, 7, 6, 9),                  # MB 1 both ways, scalar staging, K odd below one chunk, N 162: tiles cross images
    Case("c1_scalar_chunks", "c1", 6, 67, 33, 5, 5),               # fwd K 67: three chunks, kn 4, MB 2; dgrad MB 4, K 33; N 150 ragged
    Case("c1_vec_two_blocks", "c1", 9, 130, 129, 4, 4),            # vec, HW 16 < tile; grid_y 2 both ways, fwd's second block one plane; wgrad 3x3 tiles, 5 splits, last 16 px
    Case("c1_wgrad_two_chunks", "c1", 5, 260, 260, 18, 18),        # cap 40 -> klen 64: 26 splits of two chunks, last one ragged chunk; reduce 16 + 10; vec
    Case("c1_wgrad_four_chunks_scalar", "c1", 25, 520, 520, 7, 7),  # cap 12 -> klen 128: 10 splits of four chunks, last three and ragged; scalar; grid_y 5, 17 K-chunks, tail 8
    Case("gl_ragged", "gl", 11, 111, 300, G=3),                    # Kg 37, Mg 100: fwd 8 + 3; dgrad 4 + 4 + 3, three k0 chunks, tail 5
    Case("gl_strided", "gl", 4, 32, 600, G=2),                     # Kg 16 (one full chunk), Mg 300: thread stride above 256
    Case("gc_ragged", "gc", 19, 22, 38, 18, 17, G=2),              # Cg 11, Og 19: chunks 16 + 3 | 8 + 3 | 8 + 8 + 3; 306 pixels; per 2, used 10, last split one image
    Case("gc_up", "gc", 17, 9, 15, 36, 32, G=3, up=True),          # Cg 3, Og 5 from 18x16: dgrad<1> two input tiles; per 2, used 9
    Case("pm_parts", "pm", 5, 6, 6, 23, 19, G=3),                  # B L = 4370: parts 5
    Case("pm_parts_capped", "pm", 8, 6, 6, 64, 65, G=3),           # B L = 66560: parts 65 -> 64, grid-stride
    Case("pm_grid_capped", "pm", 3, 2, 2, 840, 840, G=2),          # n = 4 233 600 > 4096 x 1024
    Case("k5_wgrad_strided", "k5", 70, 20, 68, 9, 18),             # 64 splits, six with two images; 2 x 2 channel blocks with 4-plane tails; ragged tiles
]
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- inputs
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(x, gout, params [, w, b | slopes]) float32, seeded by the case name, read-only (the tests share them).  x, gradOutput ~ N(0, 1);
    weights U(-1, 1) / sqrt(fan-in); biases U(-0.5, 0.5); slopes distinct in [0.1, 0.4]; a PReLU input is sign * (0.05 + |N(0, 1)|)."""
    c = BY_NAME[name]
    rng = _rng(name)
    x = rng.standard_normal(c.in_shape, dtype=np.float32)
    gout = rng.standard_normal(c.out_shape, dtype=np.float32)
    d = dict(gout=gout)
    if c.kind == "pm":
        x = (np.where(rng.uniform(0, 1, c.in_shape) < 0.5, -1.0, 1.0) * (0.05 + np.abs(x))).astype(np.float32)
        d["slopes"] = (0.1 + 0.3 * (rng.permutation(c.G) + rng.uniform(0.1, 0.9, c.G)) / c.G).astype(np.float32)
        d["params"] = d["slopes"]
    else:
        k = {"c1": 1, "k5": 5, "gc": 3, "gl": 1}[c.kind]
        Cg = c.Cin // c.G
        wshape = (c.Cout, Cg) if c.kind == "gl" else (c.Cout, Cg, k, k)
        d["w"] = (rng.uniform(-1, 1, wshape) / np.sqrt(Cg * k * k)).astype(np.float32)
        d["b"] = rng.uniform(-0.5, 0.5, c.Cout).astype(np.float32)
        d["params"] = np.concatenate([d["w"].ravel(), d["b"]])
    d["x"] = x
    for v in d.values():
        v.setflags(write=False)
    return d


# ---------------------------------------------------------------- float64 reference and bound
# c of U * (c A + |extra|), per family of summation order.  MEASURED on the CPU with the float32 emulations below (product rounded, then the
# addition rounded: one rounding per term more than fmaf or the MFMA, so a pessimistic stand-in), largest err / (U A) over every case and
# tensor of the family against float64 (test_constants_are_twice_the_measured prints and holds them):
#   chain   a sequential chain from the bias / zero (grouplinear forward + weight gradient, groupconv3 forward + data gradient)
#   mfma    K in sequence (conv1x1 forward / data gradient), pixel runs per split then the splits' partials in split order (conv1x1 and
#           5x5 weight gradients)
#   tree    per-thread chains, a 64-lane butterfly, four waves in order [, splits in order] (grouplinear data gradient, groupconv3 weight gradient)
# MEASURED_C: chain 9.57 (groupconv3 forward behind the up-sampling: 27 products of ~0.1 onto a bias of up to 0.5 - every addition rounds
# relative to the bias, which A does not contain; without that case 5.22), mfma 5.55 (conv1x1 data gradient, K = 520), tree 0.79
# (grouplinear data gradient: one product per thread, then the tree).  c = twice the measured value (the factor covers the difference between the
# emulated and the real rounding sequence and the spread over seeds), rounded up to an integer: 20, 12, 2 -
# two of them above conv_paths.C_MODE["f32"] = 8 (measured there on one summation order and 72 .. 1152 products), so each family keeps its own.
MEASURED_C = {"chain": 9.57, "mfma": 5.55, "tree": 0.79}
C_FAMILY = {"chain": 20.0, "mfma": 12.0, "tree": 2.0, "direct": cp.C_MODE["f32"]}
# which family each tensor of each kind belongs to ("direct": the 5x5 forward / data gradient are convk_direct kernels, not emulated here:
# conv_paths.NET_CASES already holds them to its f32 constant, and so does the one 5x5 case of this table)
FAMILY = {("c1", "out"): "mfma", ("c1", "gin"): "mfma", ("c1", "gw"): "mfma", ("k5", "out"): "direct", ("k5", "gin"): "direct", ("k5", "gw"): "mfma",
          ("gl", "out"): "chain", ("gl", "gin"): "tree", ("gl", "gw"): "chain", ("gc", "out"): "chain", ("gc", "gin"): "chain", ("gc", "gw"): "tree"}


@functools.lru_cache(maxsize=None)
def reference(name):
    """{tensor: (ref, bound, A)} float64, for "out", "gin" and "gw", "gb" (or "gslope"); computed once per case and shared (read-only).
    g4_oracle.torch_reference evaluates the descriptor list twice: on the operands, and on their absolute values with a zero bias (= A, and
    for the bias gradient sum|dy|)."""
    from g4_oracle import torch_reference
    c, d = BY_NAME[name], inputs(name)
    r = torch_reference(c.descs(), c.dims, d["params"], d["x"], d["gout"])
    out = {}
    if c.kind == "pm":
        x, g = d["x"].astype(np.float64), d["gout"].astype(np.float64)
        neg = x <= 0
        assert r["kink"] >= 0.05, r["kink"]
        for key, ref in (("out", r["out"].reshape(x.shape)), ("gin", r["gin"])):
            out[key] = (ref, SLACK * U * np.where(neg, np.abs(ref), 0.0), np.abs(ref))
        prod = np.where(neg, np.abs(g * x), 0.0).reshape(c.B, c.G, -1).sum((0, 2))
        out["gslope"] = (r["grads"], SLACK * U * (prod + np.abs(r["grads"])), prod)
    else:
        pa = np.abs(d["params"]).astype(np.float64)
        pa[c.n_weights:] = 0.0
        a = torch_reference(c.descs(), c.dims, pa, np.abs(d["x"]), np.abs(d["gout"]))
        nw = c.n_weights
        bias = np.abs(d["b"]).astype(np.float64).reshape((1, -1) + (1,) * (r["out"].ndim - 2))
        cf = lambda t: C_FAMILY[FAMILY[(c.kind, t)]]
        out["out"] = (r["out"], U * (cf("out") * a["out"] + bias), a["out"])
        out["gin"] = (r["gin"], U * cf("gin") * a["gin"], a["gin"])
        out["gw"] = (r["grads"][:nw], U * (cf("gw") * a["grads"][:nw] + np.abs(r["grads"][:nw])), a["grads"][:nw])
        out["gb"] = (r["grads"][nw:], SLACK * U * (2 * a["grads"][nw:] + np.abs(r["grads"][nw:])), a["grads"][nw:])
    for t in out.values():
        for v in t:
            v.setflags(write=False)
    return out


def ratio(got, ref, bound):
    """|err| / bound per element; a zero bound (an exact copy) admits a zero error only"""
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


def check_bound(got, ref, bound, what):
    """Every element within its bound; returns max |err| / bound.  The message names the worst index (map it to chunk, split and tile with the mirror)."""
    r = ratio(got, ref, bound)
    worst = np.unravel_index(int(np.argmax(r)), r.shape)
    g = np.asarray(got).reshape(ref.shape)
    assert np.all(r <= 1.0), (f"{what}: {int((r > 1.0).sum())} of {r.size} elements outside the bound; worst at {worst}: got {float(g[worst])!r}, "
                              f"float64 {ref[worst]!r}, bound {bound[worst]:.3e} (x{r[worst]:.1f})")
    return float(r[worst])


# ---------------------------------------------------------------- float32 emulations in kernel order (CPU; the reduction index is the only loop)
def _bf16(a):
    import torch
    return torch.from_numpy(np.array(a, np.float32)).to(torch.bfloat16).float().numpy()


def _fma(acc, a, b):
    """acc + a * b in float32, the product rounded first (numpy evaluates the two ufuncs one after the other)"""
    return acc + a * b


def _block_sum_256(v):
    """group.hip block_sum_256 on axis 0 (256 threads): xor butterflies 32 .. 1 within each wave, then ((w0 + w1) + w2) + w3"""
    v = v.reshape((4, 64) + v.shape[1:])
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def emulate(name, degrade=None):
    """The case's forward, gradInput and weight gradient (or slope gradient) as float32 numpy in the kernels' summation order.
    degrade: None | "bf16" (operands rounded to bfloat16) | "drop_last_k" (forward: the last reduction index missing) | "drop_last_split"
    (weight gradient: the last split's partial missing) | "drop_second_image" (k5: the second image of the two-image splits missing) |
    "parts_layout" (pm: the partials written [part][slope], read [slope][part])."""
    c, d = BY_NAME[name], inputs(name)
    f = _bf16 if degrade == "bf16" else (lambda a: np.asarray(a, np.float32))
    x, g = f(d["x"]), f(d["gout"])
    z = lambda *s: np.zeros(s, np.float32)
    if c.kind == "pm":
        w = np.repeat(f(d["slopes"]), c.Cin // c.G)[None, :, None, None]
        m = pm_launch(c.B, c.Cin, c.H * c.W, c.G)
        prod = np.where(x > 0, np.float32(0), g * x).astype(np.float64).reshape(c.B, c.G, m["L"])
        P = np.zeros((c.G, m["parts"]))
        e = np.arange(m["total"])
        blk = (e // 256) % m["parts"]                                   # element e of a slope: workgroup (e / 256) mod gridDim.x
        for j in range(c.G):
            P[j] = np.bincount(blk, weights=prod[:, j].reshape(-1), minlength=m["parts"])
        if degrade == "parts_layout":
            P = P.T.reshape(-1).reshape(c.G, m["parts"]).copy()         # written part[blk * ns + j], read part[j * nparts + k]
        return dict(out=np.where(x > 0, x, w * x), gin=np.where(x > 0, g, w * g), gslope=P.sum(1).astype(np.float32))
    w, b = f(d["w"]), f(d["b"])
    if c.kind == "c1":
        HW, N = c.H * c.W, c.B * c.H * c.W
        X = x.reshape(c.B, c.Cin, HW).transpose(0, 2, 1).reshape(N, c.Cin)
        D = g.reshape(c.B, c.Cout, HW).transpose(0, 2, 1).reshape(N, c.Cout)
        W2 = w.reshape(c.Cout, c.Cin)
        acc = z(N, c.Cout)
        for k in range(c.Cin - (degrade == "drop_last_k")):
            acc = _fma(acc, X[:, k, None], W2[None, :, k])
        out = acc + b[None]
        acc = z(N, c.Cin)
        for o in range(c.Cout):
            acc = _fma(acc, D[:, o, None], W2[None, o, :])
        m = c1_wgrad(N, HW, c.Cin, c.Cout)
        s = z(c.Cout, c.Cin)
        for sp in range(m["splits"] - (degrade == "drop_last_split")):
            p = z(c.Cout, c.Cin)
            for n in range(sp * m["klen"], min(N, (sp + 1) * m["klen"])):
                p = _fma(p, D[n, :, None], X[n, None, :])
            s = s + p
        back = lambda t, C: t.reshape(c.B, HW, C).transpose(0, 2, 1).reshape(c.B, C, c.H, c.W)
        return dict(out=back(out, c.Cout), gin=back(acc, c.Cin), gw=s.reshape(-1))
    if c.kind == "gl":
        G, m = c.G, gl_launch(c.B, c.Cin, c.Cout, c.G)
        Kg, Mg = m["Kg"], m["Mg"]
        xr = np.repeat(x.reshape(c.B, G, Kg), Mg, axis=1)              # [B][o][k]: the inputs output o reads
        acc = np.broadcast_to(b[None], (c.B, c.Cout)).copy()
        for k in range(Kg - (degrade == "drop_last_k")):
            acc = _fma(acc, w[None, :, k], xr[:, :, k])
        out = acc
        gw = z(c.Cout, Kg)
        for bi in range(c.B):
            gw = _fma(gw, g[bi, :, None], xr[bi])
        t = np.arange(256)
        acc = z(256, c.B, G, Kg)
        gg, wg = g.reshape(c.B, G, Mg), w.reshape(G, Mg, Kg)
        for j in range(m["m_rounds"]):
            mm = t + 256 * j
            ok = mm < Mg
            gv = np.where(ok[:, None, None], gg[:, :, np.minimum(mm, Mg - 1)].transpose(2, 0, 1), np.float32(0))      # [t][B][G]
            wv = wg[:, np.minimum(mm, Mg - 1)].transpose(1, 0, 2)                                                     # [t][G][Kg]
            acc = _fma(acc, gv[..., None], wv[:, None])
        return dict(out=out, gin=_block_sum_256(acc).reshape(c.B, c.Cin), gw=gw.reshape(-1))
    if c.kind == "gc":
        G, m = c.G, gc_launch(c.B, c.Cin, c.Cout, c.G, c.H, c.W, c.up)
        Cg, Og, H, W = m["Cg"], m["Og"], c.H, c.W
        X = x.repeat(2, axis=2).repeat(2, axis=3) if c.up else x
        Xp = np.pad(X, ((0, 0), (0, 0), (1, 1), (1, 1)))
        Dp = np.pad(g, ((0, 0), (0, 0), (1, 1), (1, 1)))
        acc = np.broadcast_to(b[None, :, None, None], c.out_shape).copy()
        steps = [(ci, t) for ci in range(Cg) for t in range(9)]
        for ci, t in steps[:len(steps) - (degrade == "drop_last_k")]:
            ky, kx = divmod(t, 3)
            xs = np.repeat(Xp[:, ci::Cg, ky:ky + H, kx:kx + W], Og, axis=1)
            acc = _fma(acc, w[None, :, ci, ky, kx, None, None], xs)
        out = acc
        S = 2 if c.up else 1
        Hi, Wi = H // S, W // S
        acc = z(c.B, c.Cin, Hi, Wi)
        w5 = w.reshape(G, Og, Cg, 3, 3)
        for oc in range(Og):
            dsel = np.repeat(Dp[:, oc::Og], Cg, axis=1)                 # [B][g Cg + ci]: plane g Og + oc
            for sy in range(S):
                for sx in range(S):
                    for t in range(9):
                        ky, kx = divmod(t, 3)
                        y0, x0 = sy - ky + 2, sx - kx + 2
                        acc = _fma(acc, w5[:, oc, :, ky, kx].reshape(1, c.Cin, 1, 1), dsel[:, :, y0:y0 + S * Hi:S, x0:x0 + S * Wi:S])
        gin = acc
        hw = H * W
        P = np.stack([Xp[:, :, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], axis=2).reshape(c.B, c.Cin, 9, hw)
        Dv = g.reshape(c.B, c.Cout, hw)
        t = np.arange(256)
        s = z(c.Cout, Cg, 9)
        for sp in range(m["used"] - (degrade == "drop_last_split")):
            acc = z(256, c.Cout, Cg, 9)
            for j in range(m["pixel_rounds"]):
                p = t + 256 * j
                ok, pc = p < hw, np.minimum(p, hw - 1)
                for bi in range(sp * m["per"], min(c.B, (sp + 1) * m["per"])):
                    gv = np.where(ok[:, None], Dv[bi][:, pc].T, np.float32(0))                                        # [t][Cout]
                    xv = np.repeat(P[bi][:, :, pc].transpose(2, 0, 1).reshape(256, G, Cg, 9), Og, axis=1)             # [t][Cout][Cg][9]
                    acc = _fma(acc, gv[:, :, None, None], xv)
            s = s + _block_sum_256(acc)
        return dict(out=out, gin=gin, gw=s.reshape(-1))
    # k5: the weight gradient only (forward and data gradient are convk_direct kernels: conv_paths)
    m = k5_wgrad(c.B, c.Cin, c.Cout, c.H, c.W)
    Xp = np.pad(x, ((0, 0), (0, 0), (2, 2), (2, 2)))
    order = [(y0 + r, x0 + cx) for y0 in range(0, c.H, KW_ROWS) for x0 in range(0, c.W, KC_TILE) for r in range(KW_ROWS) for cx in range(KC_TILE)
             if y0 + r < c.H and x0 + cx < c.W]                          # tile by tile, rows, columns (pixels outside the plane add exact zeros)
    part = z(m["splits"], c.Cout, c.Cin, 5, 5)
    for rnd in range(m["max_images"] if degrade != "drop_second_image" else 1):
        nz = min(m["splits"], c.B - rnd * m["splits"])                  # splits that own an image in this round
        imgs = slice(rnd * m["splits"], rnd * m["splits"] + nz)
        for y, xx in order:
            part[:nz] = _fma(part[:nz], g[imgs, :, y, xx][:, :, None, None, None], Xp[imgs, None, :, y:y + 5, xx:xx + 5])
    s = z(c.Cout, c.Cin, 5, 5)
    for sp in range(m["splits"]):
        s = s + part[sp]
    return dict(gw=s.reshape(-1))
