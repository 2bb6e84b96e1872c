"""The nn.Linear GEMM dispatch (csrc/gemm.hip launch_gemm, csrc/net.hip fwd_linear / bwd_linear / eval_epilogue), restated; a case table
that reaches every leaf; a float64 reference and a per-element error bound in the form of conv_paths.reference.

Used by tests/test_gemm_paths_host.py (CPU: the table reaches every reachable combination, the mirror names nothing unreachable, the bound
accepts correct emulations and rejects degraded ones) and tests/test_gpu_gemm_paths.py (every case against the bound, the GEMM labels under
the per-kernel timer against the mirror).

There is no stand-alone GEMM entry point: every path is reached through a one-stage nn.Sequential holding one nn.Linear(nin, nout)
(+ nn.BatchNormalization and / or an activation in evaluate() mode for the fused epilogue):
    forward          y  = x W^T + b     M = B,    N = nout, K = nin    A = x  K-contiguous, B = W  K-contiguous, bias
    data gradient    gx = dy W          M = B,    N = nin,  K = nout   A = dy K-contiguous, B = W  N-contiguous ("strided")
    weight gradient  gW += dy^T x       M = nout, N = nin,  K = B      A = dy and B = x N- / M-contiguous ("strided"), accumulating"""
import dataclasses
import math
import zlib

import numpy as np

from conv_paths import C16, C_MODE, U, check_bound, split_terms_f16  # noqa: F401  (re-exported for the tests)

# ---------------------------------------------------------------- the dispatch, restated
MFMA, F16X3, BIG, REDUCE = "gemm_mfma_kernel", "gemm_f16x3_kernel", "gemm_f16x3_big_kernel", "gemm_splitk_reduce_kernel"
LABELS = frozenset({MFMA, F16X3, BIG, REDUCE})
POST_FORWARD = "post_forward_kernel"        # elem.hip launch_post_forward on a 1 x 1 plane (W % 4 != 0: neither the vector nor the g8 kernel)
POST_LABELS = frozenset({"post_forward_kernel", "post_forward_vec_kernel", "post_forward_g8_kernel"})
F16_MIN_WEIGHTS = 1 << 20                   # net.hip use_f16_gemm
OPS = ("fwd", "dgrad", "wgrad")


def round_up(v, m):
    return (v + m - 1) // m * m


def use_f16_gemm(mode, nin, nout):
    """net.hip use_f16_gemm: the f16x3 GEMMs for layers of at least 2^20 weights, in f16x3 mode"""
    return mode == "f16x3" and nin * nout >= F16_MIN_WEIGHTS


def gemm_plan(M, N, K, tile=64):
    """gemm.hip gemm_plan -> (nsplit, klen): split K when the output has fewer than 256 tiles, aiming at 512 workgroups with K runs of at
    least 128, rounded up to the 32-wide chunk"""
    tiles = ((M + tile - 1) // tile) * ((N + tile - 1) // tile)
    nsplit = 1
    if tiles < 256 and K >= 256:
        nsplit = max(1, min((512 + tiles - 1) // tiles, K // 128))
    klen = round_up((K + nsplit - 1) // nsplit, 32)
    return (K + klen - 1) // klen, klen


def gemm_workspace_bytes(M, N, K):
    """gemm.hip gemm_workspace_bytes: the larger of the two tilings' split counts"""
    ns = max(gemm_plan(M, N, K)[0], gemm_plan(M, N, K, 128)[0])
    return 4 * ns * M * N if ns > 1 else 0


def gemm_epilogue_possible(M, N, K):
    return gemm_plan(M, N, K)[0] == 1


@dataclasses.dataclass(frozen=True)
class Launch:
    """What one launch_gemm call does"""
    kernel: str        # MFMA, F16X3 or BIG
    nsplit: int
    klen: int
    grid: tuple        # (x, y, z)
    a_load: str        # "vec" (float4 along K), "scalar" (K-contiguous, K % 4 != 0) or "strided" (not K-contiguous)
    b_load: str
    store: frozenset   # of {"vec", "scalar"}: the store path of the 32 x 32 blocks that touch the matrix (both: within one launch)
    accumulate: bool
    bias: str          # "kernel", "reduce" or "none"
    epilogue: str      # "none" (nothing to fuse), "fused", or "refused" (split-K: the stand-alone pipeline kernel runs)

    @property
    def reduces(self):
        """launches of the reduce kernel"""
        return 1 if self.nsplit > 1 else 0

    def combo(self):
        """The leaf this launch is: (kernel, split, A load, B load, store paths, accumulate, bias place, epilogue).  The host test wants every
        one that a net can reach covered by a case."""
        return (self.kernel, self.nsplit > 1, self.a_load, self.b_load, "+".join(sorted(self.store)), self.accumulate, self.bias, self.epilogue)

    def brief(self):
        k = {MFMA: "mfma", F16X3: "f16x3", BIG: "big"}[self.kernel]
        return (f"{k} s{self.nsplit} k{self.klen} g{self.grid[0]}x{self.grid[1]} A:{self.a_load} B:{self.b_load} st:{'+'.join(sorted(self.store))}"
                f"{' acc' if self.accumulate else ''} bias:{self.bias} ep:{self.epilogue}")


def launch_gemm(M, N, K, rsA, ksA, rsB, ksB, f16, accumulate=False, bias=False, epilogue="none"):
    """gemm.hip launch_gemm (ldc = N, 16-byte aligned buffers: what net.hip passes)"""
    big = f16 and M >= 128 and N >= 128
    nsplit, klen = gemm_plan(M, N, K, 128 if big else 64)
    # the 128-tile kernel addresses a tile with 32-bit offsets from its first element
    if big and ((127.0 * rsA + (klen + 32.0) * ksA) * 4 >= 0x7FFFF000 or (127.0 * rsB + (klen + 32.0) * ksB) * 4 >= 0x7FFFF000):
        big = False
        nsplit, klen = gemm_plan(M, N, K, 64)
    if big and nsplit > 1 and gemm_epilogue_possible(M, N, K):       # "callers fuse epilogues whenever the 64-tile plan keeps K whole"
        big = False
        nsplit, klen = gemm_plan(M, N, K, 64)
    T = 128 if big else 64
    grid = ((N + T - 1) // T, (M + T - 1) // T, nsplit)

    def load(rs, ks):          # tile_load / tile_load8 / BigTileLoader: avec / bvec (kbeg = z * klen is a multiple of 32)
        if ks != 1:
            return "strided"
        return "vec" if rs % 4 == 0 and K % 4 == 0 else "scalar"

    store = set()
    if big:                    # gemm_block_vec_ok per 32 x 32 block; the 64-tile kernels only have gemm_store_block
        for mb0 in range(0, min(grid[1] * 128, round_up(M, 32)), 32):
            for nb0 in range(0, min(grid[0] * 128, round_up(N, 32)), 32):
                store.add("vec" if not accumulate and mb0 + 32 <= M and nb0 + 32 <= N and N % 4 == 0 else "scalar")
    else:
        store.add("scalar")
    assert epilogue != "fused" or nsplit == 1, "GemmArgs.ep: nsplit == 1 only"
    return Launch(BIG if big else (F16X3 if f16 else MFMA), nsplit, klen, grid, load(rsA, ksA), load(rsB, ksB), frozenset(store),
                  accumulate, ("reduce" if nsplit > 1 else "kernel") if bias else "none", epilogue)


def eval_epilogue(B, nin, nout, post, training):
    """net.hip eval_epilogue for a Linear stage without pooling, dropout or PReLU: "none" when the stage has nothing behind the Linear or the
    net trains (nothing is offered to the GEMM), else fused iff the 64-tile plan of the forward GEMM keeps K whole"""
    if not post or training:
        return "none"
    return "fused" if gemm_epilogue_possible(B, nout, nin) else "refused"


def linear_launches(mode, B, nin, nout, post=False, training=True):
    """{"fwd", "dgrad", "wgrad"} -> Launch for one nn.Linear(nin, nout) stage at batch B (net.hip fwd_linear, bwd_linear).
    From a net, two families of gemm.hip's code never run (test_gemm_paths_host.py asserts both over a grid of shapes):
      - the <AK = false, BK = true> instantiations: the only call whose A is not K-contiguous is the weight gradient, and its B is not
        either - unless nin = 1, where x's K stride nin reads as "K-contiguous" (case f32_nin1 on the fp32 kernel; the 64-tile f16x3 one
        would need nn.Linear(1, >= 2^20), no case; the 128-tile one needs N = nin >= 128: never);
      - split-K together with accumulate on either f16x3 kernel: only the weight gradient accumulates, a layer of 2^20 weights has at
        least 256 64-wide tiles in it, so its 64-tile plan never splits, and where the 128-tile plan would, launch_gemm's fall-back
        ("when callers can fuse") takes the 64-tile plan."""
    f16 = use_f16_gemm(mode, nin, nout)
    return {
        "fwd": launch_gemm(B, nout, nin, nin, 1, nin, 1, f16, bias=True, epilogue=eval_epilogue(B, nin, nout, post, training)),
        "dgrad": launch_gemm(B, nin, nout, nout, 1, 1, nin, f16),
        "wgrad": launch_gemm(nout, nin, B, 1, nout, 1, nin, f16, accumulate=True),
    }


def workspace_needed(launch, M, N):
    return 4 * launch.nsplit * M * N if launch.nsplit > 1 else 0


# ---------------------------------------------------------------- cases
ACTS = ("none", "ELU", "ReLU", "LeakyReLU", "Tanh", "Sigmoid")
LEAKY_SLOPE = 0.2


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    mode: str
    B: int
    nin: int
    nout: int
    expect: tuple          # Launch.brief() per operation, written by hand from gemm.hip (forward only for an epilogue case)
    bn: bool = False       # evaluate()-mode epilogue cases: nn.BatchNormalization behind the Linear ...
    act: str = "none"      # ... and / or an activation

    @property
    def post(self):
        return self.bn or self.act != "none"

    @property
    def ops(self):
        return ("fwd",) if self.post else OPS       # (the library refuses a backward through BatchNorm in evaluate() mode)

    @property
    def f16(self):
        return use_f16_gemm(self.mode, self.nin, self.nout)

    def launches(self):
        l = linear_launches(self.mode, self.B, self.nin, self.nout, self.post, training=not self.post)
        return {op: l[op] for op in self.ops}

    def dims(self, op):
        """(M, N, K) of the operation's GEMM"""
        return {"fwd": (self.B, self.nout, self.nin), "dgrad": (self.B, self.nin, self.nout), "wgrad": (self.nout, self.nin, self.B)}[op]


def _c(name, mode, B, nin, nout, fwd, dgrad=None, wgrad=None, **kw):
    return Case(name, mode, B, nin, nout, (fwd,) if dgrad is None else (fwd, dgrad, wgrad), **kw)


_EP_SMALL = "mfma s1 k64 g2x2 A:vec B:vec st:scalar bias:kernel ep:fused"
CASES = [
    # ---- the fp32 kernel: modes f32 and bf16x6, and f16x3 below 2^20 weights
    _c("f32_one_partial_tile", "f32", 3, 5, 7,                      # K < 32, scalar loads, one partial tile in all three operations
       "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x1 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s1 k32 g1x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f32_vec_2x2_tails", "f32", 70, 36, 65,                      # vector loads in forward, 2 x 2 grid with a 1-column and a 6-row tail, K tail of 4
       "mfma s1 k64 g2x2 A:vec B:vec st:scalar bias:kernel ep:none",
       "mfma s1 k96 g1x2 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s1 k96 g1x2 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("bf16x6_split2_scalar", "bf16x6", 5, 301, 7,                 # forward splits in 2 with scalar loads, bias through the reduce, last K run 141 = 4 * 32 + 13
       "mfma s2 k160 g1x1 A:scalar B:scalar st:scalar bias:reduce ep:none",
       "mfma s1 k32 g5x1 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s1 k32 g5x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f32_split4_vec", "f32", 33, 512, 40,                        # forward splits in 4 with vector loads; data gradient: vector A, strided B
       "mfma s4 k128 g1x1 A:vec B:vec st:scalar bias:reduce ep:none",
       "mfma s1 k64 g8x1 A:vec B:strided st:scalar bias:none ep:none",
       "mfma s1 k64 g8x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f32_wgrad_split2", "f32", 300, 40, 24,                      # weight gradient splits in 2, accumulating in the reduce onto gw0
       "mfma s1 k64 g1x5 A:vec B:vec st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x5 A:vec B:strided st:scalar bias:none ep:none",
       "mfma s2 k160 g1x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("bf16x6_wgrad_split8", "bf16x6", 1153, 65, 33,               # weight gradient splits in 8 (the reduce's unrolled loop); K % 32 == 1
       "mfma s1 k96 g1x19 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s1 k64 g2x19 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s8 k160 g2x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_mode_below_threshold", "f16x3", 40, 1023, 1025,       # 1023 * 1025 = 2^20 - 1 weights: f16x3 mode, still the fp32 kernel (and its bound)
       "mfma s7 k160 g17x1 A:scalar B:scalar st:scalar bias:reduce ep:none",
       "mfma s7 k160 g16x1 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s1 k64 g16x17 A:strided B:strided st:scalar acc bias:none ep:none"),
    # degenerate strides: launch_gemm takes "K-contiguous" from a K stride of 1, which nin = 1 or nout = 1 produce where the operand is not
    _c("f32_nin1", "f32", 3, 1, 8,                                  # nn.Linear(1, n): the weight gradient's B has K stride nin = 1 - the <AK = false, BK = true> kernel
       "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x1 A:vec B:scalar st:scalar bias:none ep:none",
       "mfma s1 k32 g1x1 A:strided B:scalar st:scalar acc bias:none ep:none"),
    _c("f32_nout1_wgrad_split2", "f32", 300, 40, 1,                 # nn.Linear(n, 1) (a discriminator's last layer): dy is K-contiguous in the weight gradient, M = 1
       "mfma s1 k64 g1x5 A:vec B:vec st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x5 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s2 k160 g1x1 A:scalar B:strided st:scalar acc bias:none ep:none"),
    # (1-wide layers: every way a stride of 1 makes launch_gemm take a strided operand for K-contiguous - never for a vector load, whose
    # row stride would have to be a multiple of 4 - unsplit and split)
    _c("f32_1_to_1_batch300", "f32", 300, 1, 1,                     # nn.Linear(1, 1): all operands "K-contiguous" scalar; weight gradient splits in 2 at M = N = 1
       "mfma s1 k32 g1x5 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x5 A:scalar B:scalar st:scalar bias:none ep:none",
       "mfma s2 k160 g1x1 A:scalar B:scalar st:scalar acc bias:none ep:none"),
    _c("f32_1_to_1_batch3", "f32", 3, 1, 1,                         # the same with the weight gradient unsplit
       "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar bias:none ep:none",
       "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar acc bias:none ep:none"),
    _c("f32_nout1_wgrad_unsplit", "f32", 3, 5, 1,                   # nn.Linear(n, 1) with the weight gradient unsplit
       "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x1 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s1 k32 g1x1 A:scalar B:strided st:scalar acc bias:none ep:none"),
    _c("bf16x6_nin1_split2_scalar", "bf16x6", 300, 1, 301,          # nn.Linear(1, n): data and weight gradient split in 2, dy through scalar loads
       "mfma s1 k32 g5x5 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s2 k160 g1x5 A:scalar B:scalar st:scalar bias:none ep:none",
       "mfma s2 k160 g1x5 A:strided B:scalar st:scalar acc bias:none ep:none"),
    _c("f32_nin1_split2_vec_a", "f32", 300, 1, 256,                 # the same with dy through vector loads
       "mfma s1 k32 g4x5 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s2 k128 g1x5 A:vec B:scalar st:scalar bias:none ep:none",
       "mfma s2 k160 g1x4 A:strided B:scalar st:scalar acc bias:none ep:none"),
    # ---- the f16x3 64-tile kernel
    _c("f16x3_split8", "f16x3", 5, 1024, 1024,                      # forward and data gradient split in 8; weight gradient on the 128-tile kernel at K = 5
       "f16x3 s8 k128 g16x1 A:vec B:vec st:scalar bias:reduce ep:none",
       "f16x3 s8 k128 g16x1 A:vec B:strided st:scalar bias:none ep:none",
       "big s1 k32 g8x8 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_unsplit_dgrad_split64", "f16x3", 3, 128, 8192,        # forward unsplit; data gradient splits in 64
       "f16x3 s1 k128 g128x1 A:vec B:vec st:scalar bias:kernel ep:none",
       "f16x3 s64 k128 g2x1 A:vec B:strided st:scalar bias:none ep:none",
       "big s1 k32 g1x64 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_ragged_everywhere", "f16x3", 37, 1030, 1100,          # scalar loads, ragged M, N and K; weight gradient on the 128-tile kernel, tails 76 and 6
       "f16x3 s7 k160 g18x1 A:scalar B:scalar st:scalar bias:reduce ep:none",
       "f16x3 s7 k160 g17x1 A:vec B:strided st:scalar bias:none ep:none",
       "big s1 k64 g9x9 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_dgrad_scalar_a", "f16x3", 37, 1030, 1101,             # nout % 4 != 0: the data gradient's K-contiguous dy through scalar loads
       "f16x3 s7 k160 g18x1 A:scalar B:scalar st:scalar bias:reduce ep:none",
       "f16x3 s7 k160 g17x1 A:scalar B:strided st:scalar bias:none ep:none",
       "big s1 k64 g9x9 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_fallback_from_128_plan", "f16x3", 256, 256, 4096,     # the 128-tile plan splits in 2, the 64-tile plan does not: forward and weight gradient fall back; data gradient in 32
       "f16x3 s1 k256 g64x4 A:vec B:vec st:scalar bias:kernel ep:none",
       "big s32 k128 g2x2 A:vec B:strided st:vec bias:none ep:none",
       "f16x3 s1 k256 g4x64 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_wgrad_fallback_k257", "f16x3", 257, 2052, 640,        # the same fall-back in the weight gradient at K = 257
       "big s13 k160 g5x3 A:vec B:vec st:scalar+vec bias:reduce ep:none",
       "big s5 k128 g17x3 A:vec B:strided st:scalar+vec bias:none ep:none",
       "f16x3 s1 k288 g33x10 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_narrow_n_split66", "f16x3", 140, 10500, 100,          # N < 128: forward on the 64-tile kernel, splits in 66 (not a multiple of 8), last K run 100
       "f16x3 s66 k160 g2x3 A:vec B:vec st:scalar bias:reduce ep:none",
       "big s1 k128 g83x2 A:vec B:strided st:scalar+vec bias:none ep:none",
       "f16x3 s1 k160 g165x2 A:strided B:strided st:scalar acc bias:none ep:none"),
    # ---- the f16x3 128-tile kernel
    _c("big_unsplit_all_vec", "f16x3", 128, 128, 8192,              # unsplit, every block through the vector store, bias in the kernel (G.fc's pattern)
       "big s1 k128 g64x1 A:vec B:vec st:vec bias:kernel ep:none",
       "big s64 k128 g1x1 A:vec B:strided st:vec bias:none ep:none",
       "big s1 k128 g1x64 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_unsplit_scalar_mixed_stores", "f16x3", 130, 102, 10300,  # scalar loads through the buffer descriptor, both store paths in one launch, 2 spare rows, 60 spare columns
       "big s1 k128 g81x2 A:scalar B:scalar st:scalar+vec bias:kernel ep:none",
       "f16x3 s65 k160 g2x3 A:vec B:strided st:scalar bias:none ep:none",
       "f16x3 s1 k160 g2x161 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_split7_scalar", "f16x3", 130, 1030, 1100,               # splits in 7, scalar loads, mixed stores into the slab
       "big s7 k160 g9x2 A:scalar B:scalar st:scalar+vec bias:reduce ep:none",
       "big s7 k160 g9x2 A:vec B:strided st:scalar bias:none ep:none",
       "big s1 k160 g9x9 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_dgrad_scalar_a", "f16x3", 130, 1030, 1101,              # the same on the 128-tile kernel's buffer-descriptor loader, K tail of 141 = 4 * 32 + 13
       "big s7 k160 g9x2 A:scalar B:scalar st:scalar bias:reduce ep:none",
       "big s7 k160 g9x2 A:scalar B:strided st:scalar bias:none ep:none",
       "big s1 k160 g9x9 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_split8_vec_slab", "f16x3", 160, 1024, 1056,             # splits in 8, all-vector slab stores, half-empty last tiles in M and N
       "big s8 k128 g9x2 A:vec B:vec st:vec bias:reduce ep:none",
       "big s7 k160 g8x2 A:vec B:strided st:vec bias:none ep:none",
       "big s1 k160 g8x9 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_split52_dgrad_unsplit", "f16x3", 129, 8200, 128,        # forward splits in 52; data gradient unsplit, 65 x 2 grid, one spare row
       "big s52 k160 g1x2 A:vec B:vec st:scalar+vec bias:reduce ep:none",
       "big s1 k128 g65x2 A:vec B:strided st:scalar+vec bias:none ep:none",
       "big s1 k160 g65x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    # ---- rows that end at M % 32 == 27 / 31: one lane half's last row (gemm_store_block: mb + 27) is the first row past the matrix - where
    # an off-by-one in `full` goes unguarded.  A row written
    # past the matrix is not something a comparison of values can see: its accumulators are zero (tile rows past M load as zero), so the
    # weight gradient would add 0 to gradBias (which follows gradWeight in the flat gradient), the forward and the data gradient would write
    # the bias / 0 behind the output buffer, and a split plan 0 into row 0 of the next split's slab, racing with that split's own store.
    _c("f32_rows_end_27_31", "f32", 31, 9, 27,
       "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "mfma s1 k32 g1x1 A:scalar B:strided st:scalar bias:none ep:none",
       "mfma s1 k32 g1x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_rows_end_27_31", "f16x3", 31, 100, 10491,             # 10491 = 327 * 32 + 27; data gradient in 66 splits with a scalar-loaded dy
       "f16x3 s1 k128 g164x1 A:vec B:vec st:scalar bias:kernel ep:none",
       "f16x3 s66 k160 g2x1 A:scalar B:strided st:scalar bias:none ep:none",
       "f16x3 s1 k32 g2x164 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_rows_end_27_31", "f16x3", 159, 6800, 155,               # 159 = 128 + 31, 155 = 128 + 27: forward in 43 splits, every block scalar (155 % 4 != 0)
       "big s43 k160 g2x2 A:vec B:vec st:scalar bias:reduce ep:none",
       "big s1 k160 g54x2 A:scalar B:strided st:scalar+vec bias:none ep:none",
       "big s1 k160 g54x2 A:strided B:strided st:scalar acc bias:none ep:none"),
    # ---- the remaining leaves (kernel x split x loads x stores x accumulate x bias x epilogue) that the cases above pass by
    _c("f32_dgrad_split4_vec_a", "f32", 33, 40, 512,                # the fp32 data gradient split in 4 with a vector-loaded dy
       "mfma s1 k64 g8x1 A:vec B:vec st:scalar bias:kernel ep:none",
       "mfma s4 k128 g1x1 A:vec B:strided st:scalar bias:none ep:none",
       "mfma s1 k64 g1x8 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_unsplit_scalar_loads", "f16x3", 3, 102, 10300,        # forward unsplit through scalar loads, K = 102 = 3 * 32 + 6
       "f16x3 s1 k128 g161x1 A:scalar B:scalar st:scalar bias:kernel ep:none",
       "f16x3 s65 k160 g2x1 A:vec B:strided st:scalar bias:none ep:none",
       "f16x3 s1 k32 g2x161 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_dgrad_unsplit_vec_a", "f16x3", 3, 8192, 128,          # data gradient unsplit (K = 128), vector dy and strided W
       "f16x3 s64 k128 g2x1 A:vec B:vec st:scalar bias:reduce ep:none",
       "f16x3 s1 k128 g128x1 A:vec B:strided st:scalar bias:none ep:none",
       "big s1 k32 g64x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("f16x3_dgrad_unsplit_scalar_a", "f16x3", 3, 8192, 130,       # the same with a scalar-loaded dy, K = 130 = 4 * 32 + 2
       "f16x3 s64 k128 g3x1 A:vec B:vec st:scalar bias:reduce ep:none",
       "f16x3 s1 k160 g128x1 A:scalar B:strided st:scalar bias:none ep:none",
       "big s1 k32 g64x2 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_unsplit_scalar_loads_all_vec", "f16x3", 128, 130, 8192,  # unsplit, scalar loads through the buffer descriptor, every block through the vector store
       "big s1 k160 g64x1 A:scalar B:scalar st:vec bias:kernel ep:none",
       "big s64 k128 g2x1 A:vec B:strided st:scalar bias:none ep:none",
       "big s1 k128 g2x64 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_unsplit_vec_loads_mixed_stores", "f16x3", 128, 100, 10500,  # unsplit, vector loads, 4 spare columns: the last block column through the scalar store
       "big s1 k128 g83x1 A:vec B:vec st:scalar+vec bias:kernel ep:none",
       "f16x3 s66 k160 g2x2 A:vec B:strided st:scalar bias:none ep:none",
       "f16x3 s1 k128 g2x165 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_split2_scalar_loads_vec_slab", "f16x3", 128, 301, 4096,  # splits in 2 with scalar loads, last K run 141, all-vector slab stores
       "big s2 k160 g32x1 A:scalar B:scalar st:vec bias:reduce ep:none",
       "big s32 k128 g3x1 A:vec B:strided st:scalar bias:none ep:none",
       "big s1 k128 g3x32 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_dgrad_unsplit_all_vec", "f16x3", 128, 8192, 128,        # data gradient unsplit, every block through the vector store
       "big s64 k128 g1x1 A:vec B:vec st:vec bias:reduce ep:none",
       "big s1 k128 g64x1 A:vec B:strided st:vec bias:none ep:none",
       "big s1 k128 g64x1 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_dgrad_unsplit_scalar_a", "f16x3", 128, 8192, 130,       # the same with a scalar-loaded dy
       "big s64 k128 g2x1 A:vec B:vec st:scalar bias:reduce ep:none",
       "big s1 k160 g64x1 A:scalar B:strided st:vec bias:none ep:none",
       "big s1 k128 g64x2 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_dgrad_split7_scalar_a_vec_slab", "f16x3", 128, 1024, 1030,  # data gradient splits in 7 with a scalar-loaded dy, all-vector slab stores
       "big s8 k128 g9x1 A:vec B:vec st:scalar bias:reduce ep:none",
       "big s7 k160 g8x1 A:scalar B:strided st:vec bias:none ep:none",
       "big s1 k128 g8x9 A:strided B:strided st:scalar acc bias:none ep:none"),
    _c("big_dgrad_split7_scalar_a_mixed_slab", "f16x3", 128, 1100, 1030,  # the same with 12 spare columns: mixed stores into the slab
       "big s7 k160 g9x1 A:vec B:vec st:scalar bias:reduce ep:none",
       "big s7 k160 g9x1 A:scalar B:strided st:scalar+vec bias:none ep:none",
       "big s1 k128 g9x9 A:strided B:strided st:scalar acc bias:none ep:none"),
    # ---- evaluate()-mode epilogue, forward only
    _c("ep_f32_bn_elu", "f32", 70, 36, 65, _EP_SMALL, bn=True, act="ELU"),
    _c("ep_f32_bn_relu", "f32", 70, 36, 65, _EP_SMALL, bn=True, act="ReLU"),
    _c("ep_bf16x6_bn_leakyrelu", "bf16x6", 70, 36, 65, _EP_SMALL, bn=True, act="LeakyReLU"),
    _c("ep_f32_bn_tanh", "f32", 70, 36, 65, _EP_SMALL, bn=True, act="Tanh"),
    _c("ep_f32_sigmoid", "f32", 70, 36, 65, _EP_SMALL, act="Sigmoid"),
    _c("ep_f32_bn_alone", "f32", 70, 36, 65, _EP_SMALL, bn=True),
    _c("ep_f16x3_bn_relu", "f16x3", 3, 128, 8192, "f16x3 s1 k128 g128x1 A:vec B:vec st:scalar bias:kernel ep:fused", bn=True, act="ReLU"),
    _c("ep_big_bn_leakyrelu_both_stores", "f16x3", 130, 102, 10300,
       "big s1 k128 g81x2 A:scalar B:scalar st:scalar+vec bias:kernel ep:fused", bn=True, act="LeakyReLU"),
    _c("ep_f16x3_split_refused", "f16x3", 5, 1024, 1024,            # the split plan: not fused, the stand-alone pipeline kernel runs
       "f16x3 s8 k128 g16x1 A:vec B:vec st:scalar bias:reduce ep:refused", bn=True, act="ReLU"),
    _c("ep_bf16x6_split_refused", "bf16x6", 5, 301, 7, "mfma s2 k160 g1x1 A:scalar B:scalar st:scalar bias:reduce ep:refused", bn=True, act="ELU"),
    _c("ep_big_split_refused", "f16x3", 130, 1030, 1100, "big s7 k160 g9x2 A:scalar B:scalar st:scalar+vec bias:reduce ep:refused", bn=True, act="Tanh"),
    # (the remaining fused and refused leaves; ELU, Tanh and Sigmoid stay on the 70 x 65 cases, where C_ACT was measured)
    _c("ep_f32_scalar_loads_bn_elu", "f32", 3, 5, 7, "mfma s1 k32 g1x1 A:scalar B:scalar st:scalar bias:kernel ep:fused", bn=True, act="ELU"),
    _c("ep_f32_split_vec_refused", "f32", 33, 512, 40, "mfma s4 k128 g1x1 A:vec B:vec st:scalar bias:reduce ep:refused", bn=True, act="LeakyReLU"),
    _c("ep_f16x3_scalar_loads_bn_leakyrelu", "f16x3", 3, 102, 10300,
       "f16x3 s1 k128 g161x1 A:scalar B:scalar st:scalar bias:kernel ep:fused", bn=True, act="LeakyReLU"),
    _c("ep_f16x3_split_scalar_refused", "f16x3", 3, 301, 4096, "f16x3 s2 k160 g64x1 A:scalar B:scalar st:scalar bias:reduce ep:refused", bn=True, act="ReLU"),
    _c("ep_big_all_vec_bn_relu", "f16x3", 128, 128, 8192,           # G.fc's evaluate() pattern: the epilogue through the LDS-transposed vector store alone
       "big s1 k128 g64x1 A:vec B:vec st:vec bias:kernel ep:fused", bn=True, act="ReLU"),
    _c("ep_big_scalar_loads_all_vec_bn", "f16x3", 128, 130, 8192, "big s1 k160 g64x1 A:scalar B:scalar st:vec bias:kernel ep:fused", bn=True),
    _c("ep_big_vec_loads_mixed_bn_leakyrelu", "f16x3", 128, 100, 10500,
       "big s1 k128 g83x1 A:vec B:vec st:scalar+vec bias:kernel ep:fused", bn=True, act="LeakyReLU"),
    _c("ep_big_split_scalar_loads_scalar_slab_refused", "f16x3", 128, 1030, 1030,
       "big s7 k160 g9x1 A:scalar B:scalar st:scalar bias:reduce ep:refused", bn=True, act="ReLU"),
    _c("ep_big_split_scalar_loads_vec_slab_refused", "f16x3", 128, 301, 4096,
       "big s2 k160 g32x1 A:scalar B:scalar st:vec bias:reduce ep:refused", bn=True, act="LeakyReLU"),
    _c("ep_big_split_vec_loads_scalar_slab_refused", "f16x3", 128, 1024, 1030,
       "big s8 k128 g9x1 A:vec B:vec st:scalar bias:reduce ep:refused", bn=True),
    _c("ep_big_split_vec_loads_mixed_slab_refused", "f16x3", 128, 512, 2052,
       "big s4 k128 g17x1 A:vec B:vec st:scalar+vec bias:reduce ep:refused", bn=True, act="ReLU"),
    _c("ep_big_split_vec_loads_vec_slab_refused", "f16x3", 128, 1024, 1024,
       "big s8 k128 g8x1 A:vec B:vec st:vec bias:reduce ep:refused", bn=True, act="LeakyReLU"),
]
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- inputs, float64 reference, bound
def inputs(case):
    """float32, seeded by the case name: x (B, nin), w (nout, nin) ~ U(-1, 1) / sqrt(nin), b ~ U(-0.5, 0.5), dy (B, nout), the accumulated
    gradients g0 = (gw0, gb0) ~ U(-1, 1); for an epilogue case also bn = (running mean, running variance, gamma, beta)"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    x = rng.standard_normal((case.B, case.nin), dtype=np.float32)
    w = (rng.uniform(-1, 1, (case.nout, case.nin)) / math.sqrt(case.nin)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, case.nout).astype(np.float32)
    dy = rng.standard_normal((case.B, case.nout), dtype=np.float32)
    gw0 = rng.uniform(-1, 1, (case.nout, case.nin)).astype(np.float32)
    gb0 = rng.uniform(-1, 1, case.nout).astype(np.float32)
    # (statistics away from the identity: mean 0 / variance 1 / gamma 1 / beta 0 would hide a swapped or dropped factor)
    bn = tuple(rng.uniform(lo, hi, case.nout).astype(np.float32) for lo, hi in ((-0.5, 0.5), (0.5, 2.0), (0.5, 1.5), (-0.5, 0.5)))
    return dict(x=x, w=w, b=b, dy=dy, gw0=gw0, gb0=gb0, bn=bn)


def operands(case, op, d):
    """(a (M, K), b (N, K)) float64: C = a b^T"""
    f = lambda t: np.asarray(t, np.float64)
    if op == "fwd":
        return f(d["x"]), f(d["w"])
    if op == "dgrad":
        return f(d["dy"]), f(d["w"]).T
    return f(d["dy"]).T, f(d["x"]).T


def reference(case, op, d, f16=None):
    """(ref, bound) float64 for the raw GEMM of the operation: |got - ref| <= U * (C_MODE A + [f16x3 kernel] C16 M) + U |extra|, per element.
    A = |a| |b|^T; M = max|a| * rowsum|b| + max|b| * rowsum|a| (conv_paths: the low fp16 term of a small entry); extra = the bias (forward)
    or the whole accumulated result (weight gradient).  A layer below 2^20 weights runs the fp32 kernel in f16x3 mode too: the fp32 bound.

    Split-K adds one fp32 addition per split (<= U/2 of a partial sum, random in sign like the accumulation errors inside a split) and is
    not given a term of its own.  MEASURED on the CPU (test_gemm_paths_host.py, emulate() against float64, max err / bound):
        K = 10500 in 66 splits (140 x 100 outputs):   fp32 0.026, f16x3 0.039
        K = 1024 in 8 splits (5 x 1024):              fp32 0.075, f16x3 0.125
        K = 512 in 4 splits (33 x 40):                fp32 0.101
        K = 102 unsplit (130 x 10300 outputs):        fp32 0.447, f16x3 0.698
    Well under half the bound at the large K, so the conv constants (measured to K = 1152) are kept; the largest ratios come from short K
    over many outputs (the maximum of 1.3 M elements whose A is small), not from long accumulations."""
    f16 = case.f16 if f16 is None else f16
    a, b = operands(case, op, d)
    ref = a @ b.T
    aa, ab = np.abs(a), np.abs(b)
    bound = (C_MODE["f16x3"] if f16 else C_MODE["f32"]) * (aa @ ab.T)
    if f16:
        bound = bound + C16 * (aa.max() * ab.sum(1)[None, :] + ab.max() * aa.sum(1)[:, None])
    if op == "fwd":
        ref = ref + np.asarray(d["b"], np.float64)[None, :]
        bound = bound + np.abs(np.asarray(d["b"], np.float64))[None, :]
    elif op == "wgrad":
        ref = ref + np.asarray(d["gw0"], np.float64)
        bound = bound + np.abs(ref)
    return ref, U * bound


def reference_grad_bias(d):
    """gradBias = gb0 + colsum dy (the pipeline backward's bias job, not a GEMM): U * (8 colsum|dy| + |result|)"""
    dy = np.asarray(d["dy"], np.float64)
    ref = np.asarray(d["gb0"], np.float64) + dy.sum(0)
    return ref, U * (8 * np.abs(dy).sum(0) + np.abs(ref))


# The evaluate()-mode epilogue (gemm.hip gemm_store_block): v = y + bias; p = ((v - mean) * invstd) * gamma + beta; out = act(p), each
# operation rounded to fp32; invstd = fp32(1 / sqrt(var + 1e-5)) computed in double (elem.hip bn_eval_prepare_kernel).
#   bound_out = L * (bound_y * |invstd gamma| + U * C_EP * (|y - mean| |invstd gamma| + |p|)) + U * C_ACT[act] * s
# L = the activation's Lipschitz constant (1; max(1, |slope|) for LeakyReLU).  C_EP: the subtraction, the two multiplications and the rounding
# of invstd are each <= U (half an ulp) relative to |y - mean| |invstd gamma| - together 4 U -, the addition of beta U |p|: 4 covers both.
# s = |out|, except on ELU's negative branch: out = expf(p) - 1 exposes the rounding of expf(p) = 1 - |out| however small |out| is
# (cancellation), which no constant times |out| covers: s = 1 = |out| + expf(p) there.
# C_ACT: expf / tanhf have no derivation in the project; MEASURED, never with the kernel: the activation in float32 numpy against float64 on
# the fp32 pre-activations of the epilogue cases below, largest |act32(p) - act64(p)| / (U s)
#     ELU 1.79   Tanh 1.81   Sigmoid 2.59   LeakyReLU 0.95 (one multiplication: <= 1)   ReLU, none 0 (exact)
# (test_activation_constants_are_twice_the_measured_error prints them and holds the constants to it); twice that, rounded up to an integer.
# For comparison, HIP documents expf at 1 ulp (2 U) and tanhf at 2 ulp (4 U): ELU <= 2 U expf(p) + U |out|, Sigmoid <= 2 U + U + U.
C_EP = 4.0
C_ACT = {"none": 0.0, "ReLU": 0.0, "LeakyReLU": 2.0, "ELU": 4.0, "Sigmoid": 6.0, "Tanh": 4.0}


def activation(act, p):
    """numpy, in p's precision"""
    one = p.dtype.type(1)
    if act == "ELU":
        return np.where(p <= 0, np.exp(np.minimum(p, 0)) - one, p)
    if act == "ReLU":
        return np.where(p > 0, p, p.dtype.type(0))
    if act == "LeakyReLU":
        return np.where(p > 0, p, p * p.dtype.type(np.float32(LEAKY_SLOPE)))
    if act == "Sigmoid":
        return one / (one + np.exp(-p))
    if act == "Tanh":
        return np.tanh(p)
    return p


def act_scale(act, p, out):
    return np.where(p <= 0, 1.0, np.abs(out)) if act == "ELU" else np.abs(out)


def epilogue64(case, d, y):
    """float64: (out, pre-activation p, y - mean, |invstd gamma|) of the case's BatchNorm + activation applied to y"""
    mean, var, gamma, beta = (np.asarray(t, np.float64) for t in d["bn"])
    if case.bn:
        invstd = 1.0 / np.sqrt(var + 1e-5)
        c, s = y - mean[None, :], (invstd * gamma)[None, :]
        p = c * s + beta[None, :]
    else:
        c, s, p = np.zeros_like(y), np.ones((1, y.shape[1])), y
    return activation(case.act, p), p, c, np.abs(s)


def reference_epilogue(case, d):
    """(ref, bound) of the stage output of an epilogue case (fused or not: the stand-alone pipeline kernel does the same arithmetic)"""
    y, by = reference(case, "fwd", d)
    out, p, c, s = epilogue64(case, d, y)
    L = max(1.0, abs(LEAKY_SLOPE)) if case.act == "LeakyReLU" else 1.0
    ep = C_EP * (np.abs(c) * s + np.abs(p)) if case.bn else 0.0
    return out, L * (by * s + U * ep) + U * C_ACT[case.act] * act_scale(case.act, p, out)


# ---------------------------------------------------------------- CPU emulations (test_gemm_paths_host.py)
def _accumulate(a, b, pairs=None, chunk=16):
    """fp32 accumulation in K order of exact products: acc = fl(acc + a[:, k] b[:, k]) (float64 product of fp32 / fp16-term values is exact;
    one rounding per addition, as a fused multiply-add).  pairs: the f16x3 kernels' term products [(i, j)] on (terms of a, terms of b), taken
    per 16-wide k step in the order given (gemm_f16x3_kernel: lo*hi, hi*lo, hi*hi)."""
    ta, tb = (a, b) if pairs else ([a], [b])
    M, K = ta[0].shape
    acc = np.zeros((M, tb[0].shape[0]), np.float32)
    for k0 in range(0, K, chunk):
        for i, j in (pairs or [(0, 0)]):
            for k in range(k0, min(K, k0 + chunk)):
                acc = (acc.astype(np.float64) + np.outer(ta[i][:, k], tb[j][:, k])).astype(np.float32)
    return acc


F16_PRODUCTS = {"f16x3": [(1, 0), (0, 1), (0, 0)], "f16x3_without_x1w0": [(0, 1), (0, 0)], "fp16_single_term": [(0, 0)]}


def emulate(case, op, d, kind="fp32", plan=None, drop_last_split=False, bias_per_split=False):
    """The operation as the kernels compute it, float32: per split of the plan (default: the mirror's) a sequential fp32 accumulation in K
    order - kind "fp32": of the fp32 operands; an F16_PRODUCTS key: of the fp16 term products of the scaled operands, scaled back by a power of
    two - then the splits added in order, then the bias / the accumulated gradient.  drop_last_split / bias_per_split: two degraded reduces."""
    import torch
    a, b = (np.ascontiguousarray(t, np.float32) for t in operands(case, op, d))
    nsplit, klen = plan or (lambda l: (l.nsplit, l.klen))(case.launches()[op])
    if kind != "fp32":
        (xa, sa), (xb, sb) = split_terms_f16(torch.from_numpy(a)), split_terms_f16(torch.from_numpy(b))
        xa, xb = [t.numpy().astype(np.float64) for t in xa], [t.numpy().astype(np.float64) for t in xb]
    bias = d["b"][None, :] if op == "fwd" else None
    total = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for z in range(nsplit - (1 if drop_last_split else 0)):
        ks = slice(z * klen, min(a.shape[1], (z + 1) * klen))
        if kind == "fp32":
            part = _accumulate(a[:, ks].astype(np.float64), b[:, ks].astype(np.float64))
        else:
            part = _accumulate([t[:, ks] for t in xa], [t[:, ks] for t in xb], F16_PRODUCTS[kind])
            part = (part.astype(np.float64) / (sa * sb)).astype(np.float32)        # ldexp: exact
        if bias_per_split and bias is not None:
            part = part + bias
        total = part if nsplit == 1 else total + part
    if bias is not None and not bias_per_split:
        total = total + bias
    if op == "wgrad":
        total = d["gw0"] + total
    return total


def emulate_epilogue(case, d, y, wrong=False):
    """gemm_store_block's epilogue on the fp32 Linear output y (bias included), float32.  wrong: gamma applied before invstd, beta dropped -
    the same value up to rounding but for the missing beta."""
    mean, var, gamma, beta = d["bn"]
    p = y
    if case.bn:
        invstd = (1.0 / np.sqrt(var.astype(np.float64) + 1e-5)).astype(np.float32)
        p = (((y - mean[None, :]) * gamma[None, :]) * invstd[None, :]) if wrong else (((y - mean[None, :]) * invstd[None, :]) * gamma[None, :] + beta[None, :])
    return activation(case.act, p.astype(np.float32))
