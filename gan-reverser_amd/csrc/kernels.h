// kernels.h — internal launch interface between the net runtime (net.hip) and the gfx950 kernels.
// Not part of the ABI (that is include/ganrev.h).
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

// ---------------------------------------------------------------- run-time selection
// The library reads four environment variables (GR_CONV_MODE, GR_RANGE_GUARD, GR_SIDE_WGRAD, GR_FUSED_HEAD: net.hip, gr_init) and answers the
// gr_set_tuning keys include/ganrev.h documents; nothing else selects kernels at run time.  Variants that lost their A/B measurement are not in
// the sources (docs/HISTORY.md names them; git has them): tools/build_base.sh + tools/ab_lib.sh compare two revisions on one machine.

namespace gr {

// ---------------------------------------------------------------- conv3x3 (implicit GEMM on fp32 MFMA)
constexpr int CONV_CK = 8;  // input channels per LDS chunk (k = tap*8 + ci_local)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }   // the launchers' test for 16-byte loads and stores

// ---------------------------------------------------------------- the row-order chain of the analysis kernels
// The reduction convention include/ganrev.h states for k-means, PCA, t-SNE, the mixture, the VAE layer and SSIM, and tests/*_paths.py restate:
// per block of ROWS_PER_BLOCK consecutive rows the values in row order from +0.0, the block partials in block order from +0.0, one division.
// The constant, the device pieces (ordered_sum8, stage_rows, block_tree_sum, below) and the mean of n doubles (chain.hip) are stated here once.
constexpr int ROWS_PER_BLOCK = 512;
constexpr long row_blocks(long n) { return (n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK; }

// ---------------------------------------------------------------- optional per-kernel HIP-event timing (bench / roofline leg)
// When a timer is installed every launch_* brackets its kernel with two events ON THE LAUNCH STREAM and reports the
// kernel's name plus its ALGORITHMIC flops and bytes; with no timer installed these are two null checks.
struct KernelTimer {
  virtual void begin(const char* name, double flops, double bytes, hipStream_t s) = 0;
  virtual void end(hipStream_t s) = 0;
  virtual ~KernelTimer() {}
};
extern KernelTimer* g_ktimer;
struct KtScope {
  hipStream_t s;
  KtScope(const char* name, double flops, double bytes, hipStream_t st) : s(st) { if (g_ktimer) g_ktimer->begin(name, flops, bytes, s); }
  ~KtScope() { if (g_ktimer) g_ktimer->end(s); }
};

// Weights in "k-major" layout consumed by conv3x3_mfma: [Cin_pad/8][9 taps][8 ci][cout_pad]
struct ConvWeightLayout {
  int cin_pad, cout_pad;
  size_t elems() const { return (size_t)cin_pad * 9 * cout_pad; }
};
inline ConvWeightLayout conv_weight_layout(int cin, int cout) {
  return ConvWeightLayout{round_up(cin, CONV_CK), round_up(cout, 32)};
}
// optional fused epilogue of the conv kernels (evaluate()-mode BatchNorm + activation); mean == nullptr: BN skipped
struct ConvEpilogue { const float *mean = nullptr, *invstd = nullptr, *gamma = nullptr, *beta = nullptr; int act = 0; float slope = 0.f; };

// f16x3 scale tracking: a slot holds bit patterns of max|tensor| (a non-negative float orders like an unsigned).  A slot is
// AMAX_ENTRIES words, each on its own 128-byte line; a producer workgroup folds its maximum into entry (linear block id %
// AMAX_ENTRIES).  Workgroups are dispatched round-robin over the 8 XCDs, so one entry is only ever touched from one XCD
// and its atomics stay in that XCD's L2 (one shared word ping-pongs between the eight L2s: measured 180 us per launch on a
// 67 MB tensor against 20 us for the kernel itself).  The slot is zeroed before the producer runs; consumers take the
// maximum over the entries.  The pre-check may read a stale (only ever smaller) value: at worst a redundant atomic.
constexpr int AMAX_ENTRIES = 32, AMAX_STRIDE = 32, AMAX_WORDS = AMAX_ENTRIES * AMAX_STRIDE;   // 4 KB per tensor slot
#if defined(__HIPCC__)
__device__ __forceinline__ void absmax_commit(float m, unsigned* slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) {
    const unsigned b = __float_as_uint(m);
    const unsigned lb = blockIdx.x + blockIdx.y * gridDim.x;
    unsigned* e = slot + (lb % AMAX_ENTRIES) * AMAX_STRIDE;
    if (b > __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(e, b);
  }
}
// maximum over the entries of a slot; every lane of a fully active wave receives it
__device__ __forceinline__ unsigned absmax_read(const unsigned* slot) {
  unsigned v = slot[(threadIdx.x & (AMAX_ENTRIES - 1)) * AMAX_STRIDE];
#pragma unroll
  for (int o = AMAX_ENTRIES / 2; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}
// Cross-lane sums on the DPP path (full-rate VALU; __shfl_xor goes through ds_bpermute and costs an LDS instruction per step:
// 13 us per conv launch for the 64 channel sums of the BatchNorm statistics against 1 us this way).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_take(float v) {      // lanes outside ROW_MASK receive 0
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
// sum over the 32 lanes of each half-wave: the result is valid in lanes 16-31 and 48-63
__device__ __forceinline__ float half_wave_sum(float v) {
  v += dpp_take<0xB1, 0xF>(v);      // quad_perm [1,0,3,2]
  v += dpp_take<0x4E, 0xF>(v);      // quad_perm [2,3,0,1]
  v += dpp_take<0x141, 0xF>(v);     // row_half_mirror: the other quad of the 8-lane half holds the same sums
  v += dpp_take<0x140, 0xF>(v);     // row_mirror: the other half of the 16-lane row
  v += dpp_take<0x142, 0xA>(v);     // row_bcast15 into rows 1 and 3: lane 15 of the row before
  return v;
}
// sum over all 64 lanes: valid in lanes 48-63
__device__ __forceinline__ float wave_sum(float v) {
  v = half_wave_sum(v);
  v += dpp_take<0x143, 0xC>(v);     // row_bcast31 into rows 2 and 3: lane 31 holds the sum of the first half-wave
  return v;
}
// v[0], v[stride], .. v[(count - 1) stride] added in that order from +0.0: eight loads in flight, then the adds in order (the joins of the chain)
__device__ __forceinline__ double ordered_sum8(const double* __restrict__ v, long count, long stride) {
  double s = 0.0;
  for (long b = 0; b < count; b += 8) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = b + u < count ? v[(b + u) * stride] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (b + u < count) s = s + t[u];
  }
  return s;
}
// Rows r0 .. r0 + nr of x [.][d] into xs [TR][ld] (ld odd: the lanes of a wave read distinct banks), element (r, c) as f(value, c), the rows past nr
// zero; by 256 threads.  The rows are one contiguous stretch of x, read 16 bytes per lane where it starts aligned; a scalar tail ends it.
struct StageAsIs { __device__ float operator()(float v, int) const { return v; } };
template <int TR, int UNROLL = 4, class F = StageAsIs>
__device__ __forceinline__ void stage_rows(const float* __restrict__ x, long r0, int nr, int d, int ld, float* xs, int tid, F f = F()) {
  const float* src = x + r0 * d;
  const int total = nr * d;
  const int total4 = (reinterpret_cast<size_t>(src) & 15) == 0 ? total & ~3 : 0;
#pragma unroll UNROLL
  for (int e = tid * 4; e < total4; e += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(src + e);
    const float vv[4] = {v.x, v.y, v.z, v.w};
    int r = e / d, c = e - r * d;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      xs[r * ld + c] = f(vv[u], c);
      if (++c == d) { c = 0; ++r; }
    }
  }
  for (int e = total4 + tid; e < TR * d; e += 256) {
    const int r = e / d, c = e - r * d;
    xs[r * ld + c] = e < total ? f(src[e], c) : 0.f;
  }
}
// The sums of NV values per thread over the NT threads of a workgroup in a fixed fp64 tree (t += t + o, o = NT / 2 .. 1); every thread gets them.
// red [NV][NT] is LDS; the leading barrier lets the call before still read it.  One barrier sequence carries all NV values.
template <int NT, int NV>
__device__ __forceinline__ void block_tree_sum(double (&v)[NV], double* red, int tid) {
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NV; ++u) red[u * NT + tid] = v[u];
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int u = 0; u < NV; ++u) red[u * NT + tid] += red[u * NT + tid + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < NV; ++u) v[u] = red[u * NT];
}
// f16x3 operand handling shared by the convolution and GEMM kernels (see conv.hip for the arithmetic)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int f16_scale_exp(unsigned amax_bits) {      // k such that max|x| * 2^k lies in [2^14, 2^15)
  const int e = (int)((amax_bits >> 23) & 0xffu);
  return e == 0 ? 0 : min(141 - e, 126);
}
__device__ __forceinline__ float pow2f(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }   // k in [-126, 127]
// split 8 scaled floats into the two fp16 term vectors (round-to-nearest both times; x - x0 is exact in fp32)
__device__ __forceinline__ void split8_f16(const float* x, float sc, uint4& t0, uint4& t1) {
  unsigned short a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = x[j] * sc;
    const _Float16 h0 = (_Float16)v; const float r = v - (float)h0; const _Float16 h1 = (_Float16)r;
    a[j] = __builtin_bit_cast(unsigned short, h0); b[j] = __builtin_bit_cast(unsigned short, h1);
  }
  t0 = make_uint4(a[0] | (unsigned)a[1] << 16, a[2] | (unsigned)a[3] << 16, a[4] | (unsigned)a[5] << 16, a[6] | (unsigned)a[7] << 16);
  t1 = make_uint4(b[0] | (unsigned)b[1] << 16, b[2] | (unsigned)b[3] << 16, b[4] | (unsigned)b[5] << 16, b[6] | (unsigned)b[7] << 16);
}
// Streaming stores (nt = true).  A plain store allocates its line in the XCD's L2 and the Infinity Cache; a non-temporal one does not.
// Round 3 measured the outputs of the convolutions, the up-sampling convolutions, the forward pipeline and pass B stored non-temporally
// in the real step, same box, interleaved: cfg3 12.62-12.86 ms, cfg2 2.059-2.066 ms - no effect beyond run-to-run noise, so every
// kernel stores plainly.  Non-temporal LOADS in the backward pipeline passes do pay at cfg3: elem.hip, ld4_maybe_nt.
typedef float st_f4 __attribute__((ext_vector_type(4)));
typedef unsigned st_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store4(float* p, const float4& v, bool nt = false) {
  if (nt) { const st_f4 t = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t, reinterpret_cast<st_f4*>(p)); }
  else *reinterpret_cast<float4*>(p) = v;
}
__device__ __forceinline__ void store4(uint4* p, const uint4& v, bool nt = false) {
  if (nt) { const st_u4 t = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t, reinterpret_cast<st_u4*>(p)); }
  else *p = v;
}
__device__ __forceinline__ float absmax4(float m, const float4& v) {
  return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}
#endif

// native [cout][cin][3][3] -> k-major (forward) ; or the transposed+flipped k-major the backward-data pass needs
void launch_conv_weight_prep(const float* w_native, float* wt, int cin, int cout, bool for_backward_data, hipStream_t s);

// out[B,Cout,H,W] = conv3x3(in) (+bias).  `up`: in is [B,Cin,H/2,W/2] and is nearest-upsampled x2 while staged.
// wt is the k-major layout for (Cin -> Cout).
// w_native (nullable): the same weights in the module's own [Cout][Cin][3][3] layout; lets few-output-channel layers
// (Cout <= 4) take the HBM-bound VALU kernel instead of a 32-row MFMA block.
void launch_conv3x3(const float* in, const float* wt, const float* bias, float* out,
                    int B, int Cin, int Cout, int H, int W, bool up, hipStream_t s, const float* w_native = nullptr,
                    const ConvEpilogue* ep = nullptr);

// Cin <= 3 forward (R's first layer): HBM-bound VALU kernel on the native weights, any arithmetic mode
bool conv_fewin_applies(int Cin, int W, bool up);
// Operand-ready OUTPUT of a convolution epilogue (evaluate() mode, f16x3; round 4).  The epilogue's result act(BN(conv)) is written
// as the consuming convolution's P16 image instead of (out == nullptr) or beside the fp32 tensor.  The image's power-of-two scale has
// to be fixed before the tensor exists: `scale` is the consumer's scale slot and already holds an UPPER BOUND of max|result|
// (launch_eval_bound: a weight-norm bound, see there); the TRUE maximum still goes to amax_out, for the bound of the stage after.
struct P16Out { void* p16 = nullptr; const unsigned* scale = nullptr; };
void launch_conv3x3_fewin(const float* in, const float* w_native, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                          hipStream_t s, const ConvEpilogue* ep = nullptr, unsigned* amax_out = nullptr,
                          double* stat_part = nullptr, int* stat_tiles = nullptr, const P16Out* p16o = nullptr);
bool conv_fewin_p16_out_supported(int Cout, int H, int W);

// fp32-accurate convolution on the bf16 MFMA: operands split into 3 bf16 terms, 6 products, fp32 accumulation ("bf16x6").
// wsplit = image made by launch_conv_weight_split (forward or backward-data flavour, like launch_conv_weight_prep).
size_t conv_weight_split_bytes(int cin, int cout, bool bwd, int ksz = 3);
// nterm 3 = bf16x6; nterm 2 = "f16x3": two fp16 terms of the power-of-two-scaled operands, 3 products.  The scales come from
// device slots holding the bit pattern of max|tensor| (amax_*), filled by launch_absmax or by the producing kernel.
void launch_absmax(const float* x, long n, unsigned* slot, hipStream_t s, bool slot_is_zero = false);   // slot_is_zero: the caller has just filled the slot with 0       // zeroes the slot, then max|x| -> slot
void launch_conv_weight_split(const float* w_native, void* dst, int cin, int cout, bool bwd, hipStream_t s, int nterm = 3, unsigned* amax = nullptr,
                              int ksz = 3, bool take_absmax = true);   // ksz 5: the 25-tap image of conv5x5_split_kernel; take_absmax false: amax already holds max|w|
// nn.SpatialConvolution(Cin, Cout, 5, 5, 1, 1, 2, 2) (models.lua:297) on the f16x3 split kernel: forward, and the data gradient with the bwd image (Cout -> Cin)
bool conv5x5_split_supported(int Cin, int Cout, int H, int W);
void launch_conv5x5_split(const float* in, const void* wsplit, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                          hipStream_t s, const unsigned* amax_in, const unsigned* amax_w);        // nterm 2: also computes amax_w
void launch_conv3x3_split(const float* in, const void* wsplit, const float* bias, float* out,
                          int B, int Cin, int Cout, int H, int W, bool up, hipStream_t s, const ConvEpilogue* ep = nullptr,
                          int nterm = 3, const unsigned* amax_in = nullptr, const unsigned* amax_w = nullptr,
                          unsigned* amax_out = nullptr /* nullable: max|out| is folded into this slot by the epilogue */,
                          // BatchNorm batch statistics from the epilogue: stat_part [Cout][tiles][2] doubles (room for
                          // conv_stat_tiles_max tiles); *stat_tiles = tiles written per channel, 0 when the kernel chosen
                          // for this shape does not produce them (then run launch_bn_stats on the output)
                          double* stat_part = nullptr, int* stat_tiles = nullptr);
// Operand-ready activations ("P16"): p16[b][c / 8][term][p16_pos(pixel)] = 16 bytes = the 8 fp16 halves of term `term` (hi, lo) of
// channels 8(c/8) .. +7 at that pixel, scaled by the power of two the tensor's scale slot defines (f16_scale_exp of its
// bits).  Same bytes as the fp32 tensor.  Written by the pipeline kernels (elem.hip), read by LDS-DMA in the conv3x3_p16_* kernels.
// Pixels are linear inside a plane: the pipeline kernels assemble the vectors through an LDS transpose (elem.hip, t8_emit), so
// consecutive lanes hold consecutive pixels and a wave's store is 1 KB contiguous.  (A "quad-major" order - pixel 4q + k at
// 64k + q, for producers whose threads own 4 pixels x 8 channels - was measured first: those threads were too heavy.)
extern int g_p16_min_tiles, g_stack8_min_wgs;
void launch_to_p16(const float* x, void* p16, int B, int C, int HW, const unsigned* slot, hipStream_t s);   // C % 8 == 0, HW % 4 == 0
#if defined(__HIPCC__)
__host__ __device__ __forceinline__ unsigned p16_pos(unsigned p) { return p; }   // position of pixel p inside a (group, term) plane: linear
#endif
bool conv_p16_supported(int B, int Cin, int Cout, int H, int W);
void launch_conv3x3_p16(const void* x_p16, const void* wsplit, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                        hipStream_t s, const ConvEpilogue* ep, const unsigned* amax_in, const unsigned* amax_w, unsigned* amax_out,
                        double* stat_part, int* stat_tiles, const P16Out* p16o = nullptr);
bool conv_p16_out_supported(int Cout);       // the P16 kernels can write their result operand-ready (whole 8-channel groups; the default four-wave kernels)
// Upper bound of max|act(BN(conv(x) + bias))| over a whole tensor BEFORE it is computed, from max|x| and the weights alone:
//   |conv_o| <= (sum_k |w_ok|) * max|x| + |bias_o|,  BatchNorm with running statistics is a per-channel affine map, and every activation
// here satisfies |act(z)| <= |z| (ELU, ReLU, LeakyReLU with |slope| <= 1) or <= 1 (Sigmoid, Tanh).  wl1 = per-output-channel L1 norms
// (launch_conv_weight_l1).  wl1 == nullptr: in_max is max|y| of the RAW main-op output (bias included) and only the pipeline is bounded.
// The bound overshoots the true maximum by a few bits (sqrt(9 Cin) x the crest factor of x); an f16x3 image scaled by a bound 2^m too large
// keeps 22 bits for elements down to 2^(m-17) of the true maximum and an absolute error of 2^(m-40) of it below - the true maximum of the
// tensor is tracked beside the bound (P16Out) so the overshoot does not compound from layer to layer.
void launch_conv_weight_l1(const float* w_native, int cout, int fan_in, float* wl1, hipStream_t s);
void launch_eval_bound(const float* wl1, const float* bias, const ConvEpilogue* ep, int Cout, float post_scale, const unsigned* in_max, unsigned* bound_out, hipStream_t s);
inline size_t conv_stat_tiles_max(int B, int H, int W) { return (size_t)B * ((H + 7) / 8) * ((W + 31) / 32) + 1; }     // smallest tile: 8 rows x 32 (or one 16x16 image)
// mean / invstd (+ running statistics) from the per-tile (sum, sum of squares) the conv epilogue wrote
// bounds (nullable): from max|y| (slot amax_y) and the fresh statistics, an upper bound of max|pipeline output| is folded into
// bound_out (the consuming convolution's scale slot) and the factor K with max|dy| <= K * max|dz| of the stage's backward
// into kb_out - both known BEFORE the kernels that write those tensors run, so they can write them operand-ready
struct BnBounds { const unsigned* amax_y; const float *gamma, *beta; int act; float mask_scale; unsigned* bound_out; unsigned* kb_out; };
void launch_bn_stats_from_tiles(const double* stat_part, int tiles, int C, double n, float* mean, float* invstd,
                                float* run_mean, float* run_var, hipStream_t s, const BnBounds* bounds = nullptr);

// nearest x2 up-sampling + conv3x3 as four 2x2 convolutions of the source plane (f16x3 arithmetic; forward only):
// 4 instead of 9 multiply-adds per output.  Shapes: source plane 8x8, 16x16 or at least 17 wide; Cout > 4.
bool conv_up2_supported(int Cin, int Cout, int H, int W);
size_t conv_weight_up2_bytes(int cin, int cout);
void launch_conv_weight_up2_split(const float* w_native, void* wup, int cin, int cout, hipStream_t s, unsigned* amax_w,
                                  bool take_absmax = true);   // take_absmax: recompute the slot max|w| first
void launch_conv3x3_up2_f16x3(const float* in, const void* wup, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                              hipStream_t s, const ConvEpilogue* ep, const unsigned* amax_in, const unsigned* amax_w, unsigned* amax_out);

// all weight images of a net in one launch
// split: 0 = fp32 k-major image, 1 = bf16 3-term image, 2 = f16 2-term image scaled by the slot `amax` (max|w|)
struct PrepJob { long w_off; void* dst; int cin, cout, CI, CO, cin_pad, cout_pad, bwd, split; unsigned* amax; };
PrepJob make_prep_job(long w_off, void* dst, int cin, int cout, bool for_backward_data, int split, unsigned* amax = nullptr);
// amax_slots != null (f16 images): the n_slots weight maxima are recomputed first
void launch_conv_weight_prep_batch(const PrepJob* jobs_dev, int njobs, const float* params, hipStream_t s,
                                   unsigned* amax_slots = nullptr, int n_slots = 0);

// weight gradient: slab workspace sized by conv_wgrad_workspace(); result accumulated (+=) into gw native layout
// mode 1: bf16x6 split on the bf16 MFMA where the shape allows (W % 8 == 0, Cin > 3); 2: f16x3 split (needs the maxima of
// x and dy in device slots); 0: fp32 MFMA
size_t conv_wgrad_workspace_bytes(int B, int Cin, int Cout, int H, int W, int mode = 0);
void launch_conv3x3_wgrad(const float* x, const float* dy, float* gw, void* workspace,
                          int B, int Cin, int Cout, int H, int W, hipStream_t s, int mode = 0,
                          const unsigned* amax_x = nullptr, const unsigned* amax_dy = nullptr);
// weight gradient with BOTH operands operand-ready (P16): x = the stage's input image, dy = pass B's image
bool conv_wgrad_p16_supported(int B, int Cin, int Cout, int H, int W);
size_t conv_wgrad_p16_workspace_bytes(int B, int Cin, int Cout, int H, int W);
void launch_conv3x3_wgrad_p16(const void* x_p16, const void* dy_p16, float* gw, void* workspace, int B, int Cin, int Cout, int H, int W,
                              hipStream_t s, const unsigned* amax_x, const unsigned* amax_dy);
inline bool conv_wgrad_is_split(int mode, int Cin, int W) { return mode >= 1 && Cin > 3 && W >= 16 && W % 8 == 0; }

// ---------------------------------------------------------------- GEMM (Linear) on fp32 MFMA
// C[m][n] (+)= sum_k A(m,k) * B(n,k) (+ bias[n]);  A(m,k) = A[m*rsA + k*ksA], B(n,k) = Bm[n*rsB + k*ksB]
size_t gemm_workspace_bytes(int M, int N, int K);
// ep (nullable; only when gemm_epilogue_possible, i.e. no split-K): per-column evaluate()-mode BatchNorm + activation
bool gemm_epilogue_possible(int M, int N, int K);
void launch_gemm(const float* A, long rsA, long ksA, const float* Bm, long rsB, long ksB,
                 float* C, long ldc, const float* bias, bool accumulate, int M, int N, int K,
                 void* workspace, hipStream_t s, const ConvEpilogue* ep = nullptr, unsigned* amax_out = nullptr,
                 // both non-null: the f16x3 kernel (operands scaled by their tracked maxima and split in two fp16 terms while staged)
                 const unsigned* amax_a = nullptr, const unsigned* amax_b = nullptr);

// ---------------------------------------------------------------- per-channel pipelines (BN / act / dropout / pool)
enum Act { ACT_NONE = 0, ACT_ELU = 3, ACT_RELU = 4, ACT_LEAKYRELU = 5, ACT_SIGMOID = 6, ACT_TANH = 7,
           ACT_PRELU = 16 /* nn.PReLU() with one shared slope: LeakyReLU whose slope is read from device memory (PostArgs::slope_dev) */ };
enum MaskKind { MASK_NONE = 0, MASK_ELEM = 1, MASK_SPATIAL = 2, MASK_SCALE = 3 /* evaluate(): x*(1-p) */ };
struct MaskRef { int kind; const uint32_t* bits; float scale; };
enum PoolMode { POOL_NONE = 0, POOL_MAX = 1 /* nn.SpatialMaxPooling(2,2) */, POOL_AVG = 2 /* nn.SpatialAveragePooling(2,2,2,2): no index */ };

struct PostArgs {
  const float* y;          // raw main-op output [B,C,H,W]
  float* out;              // pipeline output [B,C,Ho,Wo]
  int B, C, H, W;          // pre-pool dims
  int has_bn;
  const float *mean, *invstd, *gamma, *beta;  // per channel
  int act; float slope;
  const float* slope_dev;  // ACT_PRELU: the learnable slope (one float in the net's flat parameter vector)
  MaskRef m1;              // applied before the pool, indexed at [B,C,H,W] (ELEM) or [B,C] (SPATIAL)
  int pool;                // PoolMode: none, or a 2x2 pool of stride 2 (max or average)
  uint8_t* pool_idx;       // [B,C,Ho,Wo] argmax 0..3 (POOL_MAX only; null for POOL_AVG)
  MaskRef m2;              // applied after the pool, indexed at [B,C,Ho,Wo] / [B,C]
  unsigned* amax_out;      // nullable: max|out| is folded into this slot (f16x3 scale of the consuming convolution)
  // operand-ready copy of `out` for the convolution that consumes it (see conv_p16_supported): p16 != null selects the
  // 8-channel-group kernel; p16_scale = the consumer's scale slot, which already holds an UPPER BOUND of max|out| (written by
  // launch_bn_stats_from_tiles from the batch statistics and max|y|) - amax_out must then be null
  void* p16; const unsigned* p16_scale;
  int nt;                  // non-temporal loads of y (set by the launcher: tensors far larger than the Infinity Cache)
  int nt_st;               // non-temporal stores of the outputs (0 at every launch: kernels.h store4)
};
void launch_post_forward(const PostArgs& a, hipStream_t s);

constexpr int PB_SPLITS = 256;   // row length of partials_b: pass B of the operand-ready pipeline slices the batch finer than pass A (blocks of 8 channels)
constexpr int STAT_SPLITS = 64;  // partial sums per channel (16 -> 64: 4 -> 16 waves per SIMD in flight on the 64-channel layers; pass A 1.41 -> 1.12 ms at cfg3)
// per-channel (sum, sumsq) partials in double -> mean / invstd (+ running stats update when run_mean != null)
// Synchronised BatchNorm under data parallelism (optional): the per-channel sums a BatchNorm layer reduces over its batch -
// (sum y, sum y^2) in the forward, (sum dz, sum dz (y - mean)) in the backward - are added over the ranks before they are used, so
// that P ranks of B images compute exactly what one device computes on P x B images (models.lua:410-448 on the global batch).
// `sum` is called in stream order with a compact device buffer [count] of doubles and must leave the SUM over the ranks in it;
// `max_u32` likewise with the element-wise maximum (the f16x3 scale bound of dy needs the GLOBAL max|dz|).  n_global = elements per
// channel over all ranks; grad_scale = 1 / ranks for the gamma / beta gradients, which come out of the GLOBAL sums on every rank and
// meet the gradient all-reduce (a SUM) afterwards.
struct StatSync {
  int (*sum)(void* user, double* buf, long count);
  int (*max_u32)(void* user, unsigned* buf, long count);
  void* user;
  double* buf;             // device scratch, >= 2 * C doubles
  double n_global;
  float grad_scale;
};
// per-channel sums of `count` (a, b) pairs at row stride `stride` pairs -> compact out[C][2]  (fixed order: deterministic)
void launch_pair_sums(const double* part, int stride, int count, int C, double* out, hipStream_t s);
// out[C][2] -> pair 0 of every row of a [C][stride][2] array
void launch_pair_scatter(const double* in, int C, int stride, double* part, hipStream_t s);
void launch_bn_stats(const float* y, int B, int C, int HW, double* partials /*[C][STAT_SPLITS][2]*/,
                     float* mean, float* invstd, float* run_mean, float* run_var, int training, hipStream_t s, const StatSync* sync = nullptr);
void launch_bn_eval_prepare(const float* run_mean, const float* run_var, float* mean, float* invstd, int C, hipStream_t s);

struct PostBwdArgs {
  PostArgs f;              // the forward description (y, masks, pool_idx, bn params)
  const float* gout;       // grad wrt pipeline output [B,C,Ho,Wo]
  float* dy;               // grad wrt raw y [B,C,H,W] (written)
  double* partials;        // [C][STAT_SPLITS][2]
  float* coef;             // [C][2] : gm, k   (BN backward coefficients)
  float* ggamma; float* gbeta;   // += (BN)
  float* gbias;            // += sum dy per channel (conv / linear bias), nullable
  unsigned* amax_dy;       // nullable: max|dy| is folded into this slot (f16x3 scale of the weight / data gradients)
  double* partials_b;      // [C][PB_SPLITS] pass B's per-channel sums of dy (bias gradient); separate from `partials`,
                           // which every pass-B workgroup of the channel still reads (BN coefficients are derived in pass B)
  // operand-ready copy of dy for the data-gradient convolution: dy_p16 != null selects the 8-channel-group pass B.  amax_dz
  // receives max|dz| from pass A; kb holds the forward's factor K (BnBounds); pass B writes the bound K * max|dz| into amax_dy
  // (which then must not be accumulated into) and scales by it.
  void* dy_p16; unsigned* amax_dz; const unsigned* kb;
  int nt;                  // non-temporal loads of gradOutput and y (set by the launcher, per pass)
  double gscale;           // factor on the gamma / beta gradients: 1, or 1 / ranks under synchronised BatchNorm (StatSync); 0 reads as 1
};
bool post_g8_supported(int C, int H, int W, bool pool, bool backward = false);
// Bias gradients are summed from partials_b by one batched launch for several stages (launch_bias_grad_batch) when
// `defer` is given; otherwise inside the call.
struct BiasJob { const double* partials; float* gbias; int C, splits; };     // partials: rows of PB_SPLITS
struct BiasJobs { BiasJob job[16]; int n; };
void launch_post_backward(const PostBwdArgs& a, hipStream_t s, BiasJobs* defer = nullptr, const StatSync* sync = nullptr);
void launch_bias_grad_batch(BiasJobs& jobs, hipStream_t s);    // runs and empties the list
// evaluate()-mode backward of the pipeline in ONE pass (nn.Module:updateGradInput with a frozen BatchNorm): dy = dz * (invstd * gamma)[c], where
// mean / invstd are launch_bn_eval_prepare's.  Reads f, gout, dy and amax_dy of the argument block; no partials, no coef, no parameter gradient.
void launch_post_backward_frozen(const PostBwdArgs& a, hipStream_t s);

// ---------------------------------------------------------------- K x K convolution (odd K other than 3) and nn.PReLU: convk.hip
bool convk_supported(int K);
size_t convk_workspace_bytes(int B, int Cin, int Cout, int K);
void launch_convk_forward(const float* in, const float* w /*[Cout][Cin][K][K]*/, const float* bias, float* out, void* ws, int B, int Cin, int Cout, int H, int W, int K, hipStream_t s);
void launch_convk_backward_data(const float* gout, const float* w, float* gin, void* ws, int B, int Cin, int Cout, int H, int W, int K, hipStream_t s);
void launch_convk_backward_weight(const float* in, const float* gout, float* gw /*+=*/, void* ws, int B, int Cin, int Cout, int H, int W, int K, hipStream_t s);
// the 1 x 1 window (conv1x1.hip): batched GEMMs over the pixels of the whole batch on the fp32 MFMA; launch_convk_* dispatch K == 1 here
size_t conv1x1_workspace_bytes(int B, int Cin, int Cout);
void launch_conv1x1_forward(const float* in, const float* w /*[Cout][Cin]*/, const float* bias, float* out, int B, int Cin, int Cout, int HW, hipStream_t s);
void launch_conv1x1_backward_data(const float* gout, const float* w, float* gin, int B, int Cin, int Cout, int HW, hipStream_t s);
void launch_conv1x1_backward_weight(const float* in, const float* gout, float* gw /*+=*/, void* ws, int B, int Cin, int Cout, int HW, hipStream_t s);
size_t prelu_grad_workspace_bytes();
void launch_prelu_grad(const float* g, const float* z, long n, double* part, float* gslope /*+=*/, hipStream_t s);

// ---------------------------------------------------------------- grouped layer kinds (group.hip): exact fp32 in every mode, deterministic (GR_GROUPCONV3 also: groupmfma.hip)
// GR_GROUPLINEAR: x [B][a], w [b][a/G], y [B][b]; group g maps inputs [g a/G, (g+1) a/G) to outputs [g b/G, (g+1) b/G)
void launch_grouplinear_forward(const float* x, const float* w, const float* bias, float* y, int B, int a, int b, int G, hipStream_t s);
void launch_grouplinear_backward_data(const float* gout, const float* w, float* gin, int B, int a, int b, int G, hipStream_t s);
void launch_grouplinear_backward_weight(const float* x, const float* gout, float* gw /*+=*/, int B, int a, int b, int G, hipStream_t s);
// GR_GROUPCONV3: w [Cout][Cin/G][3][3]; H x W are the convolution's planes; up: in / gin are [B][Cin][H/2][W/2] (nearest x2 up-sampling indexed in place)
size_t groupconv3_workspace_bytes(int B, int Cin, int Cout, int G);
void launch_groupconv3_forward(const float* in, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int G, int H, int W, bool up, hipStream_t s);
void launch_groupconv3_backward_data(const float* gout, const float* w, float* gin, int B, int Cin, int Cout, int G, int H, int W, bool up, hipStream_t s);
void launch_groupconv3_backward_weight(const float* in, const float* gout, float* gw /*+=*/, void* ws, int B, int Cin, int Cout, int G, int H, int W, bool up, hipStream_t s);
#if defined(__HIPCC__)
__global__ void group_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, long n, int splits);   // gw[e] += the splits' partials in split order
#endif
// GR_GROUPCONV3 on the f16 / bf16 MFMA (groupmfma.hip): same tensors, results fp32-accurate in the split arithmetic of `mode` (2 = f16x3 with a scale per
// (image, group) tile, else bf16x6), deterministic.  Supported: 16 planes per group on both sides, H, W <= 32; ws = groupconv3_workspace_bytes
extern int g_group_mfma_min_tiles;       // gr_set_tuning "group_mfma_min_tiles": (image, group) tiles from which net.hip takes these launches
bool groupconv3_mfma_supported(int Cin, int Cout, int G, int H, int W, bool up);
void launch_groupconv3_mfma_forward(const float* in, const float* w, const float* bias, float* out, int B, int G, int H, int W, bool up, int mode, hipStream_t s);
void launch_groupconv3_mfma_backward_data(const float* gout, const float* w, float* gin, int B, int G, int H, int W, bool up, int mode, hipStream_t s);
void launch_groupconv3_mfma_backward_weight(const float* in, const float* gout, float* gw /*+=*/, void* ws, int B, int G, int H, int W, bool up, int mode, hipStream_t s);
// GR_PRELU with ns >= 2 slopes over [B][C][HW]: slope j covers channels [j C/ns, (j+1) C/ns)
void launch_prelu_multi_forward(const float* x, const float* w, float* y, int B, int C, int HW, int ns, hipStream_t s);
void launch_prelu_multi_backward(const float* g, const float* x, const float* w, float* gin, int B, int C, int HW, int ns, hipStream_t s);
size_t prelu_multi_grad_workspace_bytes(int ns);
void launch_prelu_multi_grad(const float* g, const float* x, int B, int C, int HW, int ns, double* part, float* gw /*+=*/, hipStream_t s);

// ---------------------------------------------------------------- criterion / optimiser / misc
void launch_mse(const float* x, const float* t, long n, long n_global, double* loss_dev, float* grad, hipStream_t s);
// R's head in one launch (elem.hip, head_fwd_bwd_kernel): BatchNorm + act + Dropout of the fc1 stage, fc2 [+ Tanh], MSE, and their backward down to fc1's dy
struct HeadLaunch {
  int B, C1, nd; long n_global;
  const float* y1; float* out1;                                  // fc1: raw output (bias added), stage output
  float *mean, *invstd, *run_mean, *run_var; const float *gamma, *beta;
  MaskRef m1; int act1; float slope1; int act2;                  // fc1 stage: Dropout mask, activation; fc2 stage: ACT_NONE or ACT_TANH
  const float *W2, *b2; float *y2, *out2;                        // fc2: weights [nd][C1], bias, raw output, stage output (== y2 without an activation)
  const float* target; double* loss; double* loss_part;          // the criterion's target, device loss, [C1 / 8] partial sums
  float *gout, *gy2, *dy1;                                       // gradOutput of the net [B][nd], gradient wrt fc2's raw output, wrt fc1's raw output [B][C1]
  float *gW2, *gb2, *ggamma, *gbeta, *gb1;                       // accumulated into (accGradParameters)
  unsigned* amax_dy;                                             // f16x3: max|dy1| slot of fc1's backward GEMMs (nullable)
  unsigned* bar; unsigned bar_base;                              // grid-barrier arrival counter (monotonic; the launch adds 2 x C1 / 8) and its value before this launch
  unsigned* fault; int spin_limit;                               // sticky fault word a timed-out barrier sets; polls per barrier before giving up (0 = the default 2^22, ~5 s)
};
bool head_supported(int B, int C1, int nd);
void launch_head_fwd_bwd(const HeadLaunch& h, hipStream_t s);
void launch_add_inplace(float* y, const float* x, long n, hipStream_t s);        // y += x
void launch_bce(const float* x, const float* t, long n, double* loss_dev, float* grad, hipStream_t s);      // nn.BCECriterion (sizeAverage)
struct AdamConsts { float b1, b2, c1, c2, eps, step, l1, l2, clamp; int use_penalty, use_clamp; };
void launch_penalty_clamp_adam(float* theta, float* g, float* m, float* v, long n, const AdamConsts& c, hipStream_t s, const unsigned* skip = nullptr);
// optim.adam's scalars at step t (1-based): the step size in double, rounded to fp32 once; epsilon stays outside the bias correction
inline AdamConsts adam_consts_plain(double lr, double beta1, double beta2, double eps, int t) {
  AdamConsts k{};
  k.b1 = (float)beta1; k.b2 = (float)beta2; k.eps = (float)eps;
  k.c1 = (float)(1.0 - beta1); k.c2 = (float)(1.0 - beta2);
  const double bc1 = 1.0 - std::pow(beta1, t), bc2 = 1.0 - std::pow(beta2, t);
  k.step = (float)(-(lr * std::sqrt(bc2) / bc1));
  return k;
}
// noise refinement (elem.hip): per-row MSE with its gradient (grad nullable), and best-keeping + Adam on [rows][nd] in one launch each
void launch_mse_rows(const float* x, const float* t, long rows, long n, float* loss_rows, float* grad, hipStream_t s);
void launch_adam_rows(float* z, float* g, float* m, float* v, int rows, int nd, const AdamConsts& c, float zclamp, const float* loss_rows, float* best_loss,
                      float* best_z, int update, hipStream_t s);
// The optim rock's other five methods (adversarial.lua:147-161,174-188), same fused pass.  method = GR_OPT_* (net.hip asserts the two lists agree).
// Every scalar is rounded to fp32 once on the host (gr_optim_step); a method reads only its own: sgd lr (= clr), wd, mom, omd (1 - dampening), use_wd,
// use_mom, nesterov, first (t == 1: the buffer becomes the gradient); adagrad lr (= clr); adadelta rho, omr (1 - rho), eps; adamax b1, c1 (1 - beta1),
// b2, eps, lr (= lr / (1 - beta1^t)); rmsprop lr, rho (alpha), omr (1 - alpha), eps.
enum { OPT_SGD = 1, OPT_ADAGRAD = 2, OPT_ADADELTA = 3, OPT_ADAMAX = 4, OPT_RMSPROP = 5 };
struct OptimConsts { float lr, wd, mom, omd, rho, omr, eps, b1, c1, b2, l1, l2, clamp; int use_wd, use_mom, nesterov, first, use_penalty, use_clamp; };
void launch_penalty_clamp_optim(int method, float* theta, float* g, float* s0, float* s1, long n, const OptimConsts& c, hipStream_t s, const unsigned* skip = nullptr);
void launch_gen_mask(uint32_t* words, long n_elems, float p_drop, uint64_t seed, uint64_t counter, uint32_t layer, hipStream_t s);
// all masks of one forward in one launch (jobs travel in the kernel argument block)
struct MaskJob { uint32_t* words; long nwords; uint32_t thresh; int half; uint32_t layer; };
struct MaskJobs { MaskJob job[24]; int n; };
MaskJob make_mask_job(uint32_t* words, long n_elems, float p_drop, uint32_t layer);
void launch_gen_mask_batch(const MaskJobs& jobs, uint64_t seed, uint64_t counter, hipStream_t s);
void launch_pack_mask(const uint8_t* keep, uint32_t* words, long n, hipStream_t s);
void launch_unpack_mask(const uint32_t* words, uint8_t* keep, long n, hipStream_t s);
void launch_fill_normal(float* dst, long n, uint64_t seed, hipStream_t s);
void launch_fill_uniform(float* dst, long n, float lo, float hi, uint64_t seed, hipStream_t s);

// ---- f16x3 range guard.  The f16x3 arithmetic scales a whole tensor by one power of two: an entry 2^k below the tensor's
// maximum keeps about 40 - k bits (fp16's exponent range ends there).  Where a kernel's reduction runs over a channel index (the
// forward and the data gradient: activation x weight), the worst-case relative error of an output channel grows with the PRODUCT
// of the two tensors' per-channel spreads; where it runs over pixels (the weight gradient: activation x gradient, one channel
// pair per sum) with the larger one.  These kernels measure spreads: per-channel max|.| of a strided view t[b * sB + c * sC + i]
// (b < B, i < HW) into chmax[c] (atomicMax of bit patterns; chmax must be zero), then one verdict block enters
// log2(max_c / smallest non-zero chmax) (+1) into the largest spread seen so far on its SIDE - *word = activation side (0) |
// weight side (1) << 16 - and zeroes chmax again.  launch_pair_spread does the same, activation side, for the per-channel vector
// max(|a_c|, |b_c|) (BatchNorm gamma / beta: they set the channel ranges of every tensor behind a BatchNorm).  The caller compares
// the sum of the two sides with its budget (net.hip: 20 bits).
void launch_channel_absmax(const float* t, int B, int C, long HW, long sB, long sC, unsigned* chmax, hipStream_t s);
void launch_spread_verdict(unsigned* chmax, int C, unsigned* word, int side, hipStream_t s);
void launch_pair_spread(const float* a, const float* b, int C, unsigned* word, hipStream_t s);
void launch_l2_distance_rows(const float* a, const float* b, long n, long d, double* out, hipStream_t s);
void launch_scale_copy(const float* src, float* dst, long n, float scale, hipStream_t s);
// NN_UTILS.switchColorSpace (utils/nn_utils.lua:133-246): in [batch x (1|3) x hw] -> out [batch x (1|3) x hw], from / to = GR_CS_*; one launch,
// none for rgb -> rgb.  A 16-byte form when hw % 4 == 0 and both pointers are 16-byte aligned, a scalar form otherwise.
enum { CS_RGB = 0, CS_Y = 1, CS_YUV = 2, CS_HSL = 3 };
void launch_colorspace(const float* in, int from, int to, long batch, long hw, float* out, hipStream_t s);
// ---- dataset.lua's per-image work (dataset.hip; include/ganrev.h, gr_image_scale_dev / gr_dataset_images_dev, states the arithmetic).
// ScaleAxis = one pass of image.scale's scaleLinear_rowcol(src_len, dst_len); scale is one correctly rounded fp32 division of two exact
// conversions, on the host - or, by the same function, in the gather kernel, whose source sizes differ from image to image.
enum { SCALE_COPY = 0, SCALE_UP = 1, SCALE_DOWN = 2, SCALE_REPLICATE = 3 };
struct ScaleAxis { int mode, src_len, dst_len; float scale; };
constexpr int SCALE_MAX_LEN = 32768;                               // per side: keeps every fp32 index product below 2^15, far from an integer it must not reach
__host__ __device__ inline ScaleAxis scale_axis(int src_len, int dst_len) {
  if (dst_len == src_len) return ScaleAxis{SCALE_COPY, src_len, dst_len, 1.f};
  if (dst_len < src_len) return ScaleAxis{SCALE_DOWN, src_len, dst_len, (float)src_len / (float)dst_len};
  if (src_len == 1) return ScaleAxis{SCALE_REPLICATE, src_len, dst_len, 0.f};
  return ScaleAxis{SCALE_UP, src_len, dst_len, (float)(src_len - 1) / (float)(dst_len - 1)};
}
// in [nplanes x sh x sw] -> out [nplanes x dh x dw]; ay = scale_axis(sh, dh), ax = scale_axis(sw, dw).  One launch; 16-byte stores when dw % 4 == 0
// and out is 16-byte aligned, a scalar form otherwise.
void launch_image_scale(const float* in, long nplanes, const ScaleAxis& ay, const ScaleAxis& ax, float* out, hipStream_t s);
// in uint8 [n x sh x sw x sc] (sc 1, 3 or 4) -> out [n x (1|3) x dh x dw] in colour space `to`, normalised to [-1, 1] when normalize != 0.  One launch.
void launch_dataset_images(const uint8_t* in, long n, int sc, const ScaleAxis& ay, const ScaleAxis& ax, int to, int normalize, float* out, hipStream_t s);
// The same per image over a cache of decoded files of mixed size (gr_dataset_cache_*): row k of out [n x (1|3) x dh x dw] is what
// launch_dataset_images writes for image recs[idx[k]] alone.  CachedImage = where an image's bytes lie (4-byte aligned, padded to a dword,
// at least one more dword of the allocation behind them) and its source size.  One launch whatever sizes the list mixes; bytes_in = the
// bytes of the listed images (the timer's label).  The caller has checked every idx[k] against the record count.
struct CachedImage { const uint8_t* data; int sh, sw, sc, pad; };
void launch_dataset_gather(const CachedImage* recs, const long* idx, long n, int dh, int dw, int to, int normalize, float* out, double bytes_in, hipStream_t s);
// ---- image grids (render.hip): image.toDisplayTensor over tiles gathered from device-resident image tables, with the decorations of
// apply_r.lua's pictures (include/ganrev.h, gr_image_grid_dev, states the arithmetic).  GridTile is the per-tile metadata the kernels read
// from a small device array; GridGeom travels in the kernel arguments.
struct GridTile { long row[2]; float bg[3]; int inset; };          // row[s] = -1: slot s shows the background
struct GridGeom {
  const float* src[2]; const GridTile* tiles;
  int slots, C, Cout, H, W, from;                                  // from = CS_* or -1 (channels copied as they are)
  int n_tiles, xmaps, padding, margin, TH, TW, cellH, cellW, GH, GW;
  float inset_rgb[3], fill, lo, hi;
};
constexpr int GRID_RANGE_BLOCKS = 256;                             // upper bound of the (min, max) partial pairs of an auto-range grid
// parts != null: auto range - image_grid_range_kernel leaves up to GRID_RANGE_BLOCKS (min, max) pairs over every pixel inside a tile in
// parts [2 x GRID_RANGE_BLOCKS floats], the grid kernel reduces them to lo / hi; null: g.lo / g.hi.  One launch, two with auto range.
void launch_image_grid(const GridGeom& g, float* parts, float* grid, uint8_t* u8, hipStream_t s);
// ---- the trainers' progress pictures (render.hip): NN_UTILS.imagesToGridTensor (utils/nn_utils.lua:490-548) from a device-resident table;
// include/ganrev.h, gr_progress_grid_dev, states the layout.  rows: device array of the n_cells rows shown; dig: the epoch's decimal digits,
// least significant first.
struct ProgressGeom {
  const float* src; const long* rows;
  int C, Cout, H, W, from;                                         // from = CS_* or -1 (channels copied as they are)
  int n_cells, grid_w, GH, GW, ndig;
  unsigned char dig[12];
};
// vec: four pixels of a row per thread (the caller has checked W % 4 == 0 and the alignment of src, grid and u8), else one.  One launch.
void launch_progress_grid(const ProgressGeom& g, bool vec, float* grid, uint8_t* u8, hipStream_t s);
// out[p] = (((0 + x[rows[0]][p]) + x[rows[1]][p]) + ...) / n for p < d, rows a device array; n == 0: zeros
void launch_rows_mean(const float* x, long d, const long* rows_dev, int n, float* out, hipStream_t s);
// several regions zeroed by ONE launch (each a multiple of 16 bytes, 16-byte aligned): the fills a training step needs - the scale slots of both
// nets, the gradient vector - were three hipMemsetAsync kernels of ~6 us each at batch 256
struct ZeroJobs { void* ptr[4]; long n16[4]; int n; };
void launch_zero_regions(const ZeroJobs& jobs, hipStream_t s);
void launch_upsample2(const float* x, float* up, int B, int C, int Ho, int Wo, hipStream_t s);       // nearest x2, [B,C,Ho/2,Wo/2] -> [B,C,Ho,Wo]
void launch_downsum2(const float* gup, float* gin, int B, int C, int Hs, int Ws, hipStream_t s);   // its backward: sum of each 2x2 block

// ---------------------------------------------------------------- cosine top-k search
size_t cosine_topk_workspace_bytes(long N, int d, int Q, int k);
// idx_out/score_out are DEVICE buffers [Q][k].  status_dev (device word, nullable): large tables take the sample-bound filter
// (search.hip) when it is given; it receives 1 when a candidate list overflowed - call again with unfiltered = 1 - else 0.
// query_rows_host (nullable): the same rows in host memory - a handful of needles (cosine_topk_small_path) travel in the kernel arguments
int launch_cosine_topk(const float* emb, long N, int d, const long* query_rows_dev, int Q, int k,
                       long* idx_out, float* score_out, int accf, void* workspace, hipStream_t s, unsigned* status_dev = nullptr, int unfiltered = 0,
                       const long* query_rows_host = nullptr, unsigned* arrival_counter = nullptr,    // arrival_counter: SEARCH_STATE_WORDS zeroed device words the caller owns (word 0: the sample launch's arrival counter, words 16..: its histogram bins; both are left at 0 again)
                       unsigned* done_words = nullptr, unsigned seq = 0,    // small path: done_words[q] (host-visible) receives seq once needle q's results are written; the call then returns 2
                       const float* queries_dev = nullptr);   // non-null: needle q is row q of this device array [Q][d] (a vector from outside the table) and both query_rows are unused
constexpr int SEARCH_STATE_WORDS = 16 + 8 * 1024;
bool cosine_topk_small_path(long N, int d, int Q, int k);     // the filtered search takes the fp32-filter path (query rows by value, no device copy of them needed)

// ---------------------------------------------------------------- exact L2 nearest neighbours (sample.lua:130-148; neighbours.hip)
size_t l2_nearest_workspace_bytes(long n, int Q);
bool l2_nearest_direct(long n);          // small tables: the exact path outright
double l2_filter_eps(int d, bool vec);   // relative bound |S~ - S| <= eps S of the streaming pass
// x [n][d], qs [Q][d], idx_out / dist_out [Q][k], status [Q]: all device.  exact = 0: streaming pass + candidate selection; status[q] = 1 means
// query q's candidate list overflowed and the call must be repeated with exact = 1 (every row scored exactly; status untouched).  Returns -1
// for a shape outside 1 <= d <= 65536, 1 <= k <= min(128, n).
int launch_l2_nearest(const float* x, long n, int d, const float* qs, int Q, int k, long* idx_out, double* dist_out, unsigned* status,
                      void* workspace, int exact, int num_cus, hipStream_t s);

// ---------------------------------------------------------------- the mean of n doubles by the row-order chain (chain.hip)
// out[0] = ((the rows of each block of ROWS_PER_BLOCK in row order from +0.0), the block partials in block order from +0.0) / n.  rows [n], part
// [row_blocks(n)], out: device; a caller's scratch for rows and part is chain_mean_doubles(n) doubles.  One launch when n <= ROWS_PER_BLOCK, else two,
// inside one KtScope named `timer`.
inline size_t chain_mean_doubles(long n) { return (size_t)n + (size_t)row_blocks(n); }
inline size_t chain_mean_workspace_bytes(long n) { return sizeof(double) * chain_mean_doubles(n) + 256; }
void launch_chain_mean(const double* rows, long n, double* part, double* out, const char* timer, hipStream_t s);

// ---------------------------------------------------------------- k-means + nearest-centroid pass (apply_r.lua:197-217)
size_t kmeans_workspace_bytes(long N, int d, int k);
// all pointers device; cent [k][d] holds the initial centroids on entry and the final ones on return; returns 1 when the
// shape is unsupported (k > 32, d > 256)
int launch_kmeans(const float* x, long N, int d, int k, int niter, float* cent, float* c2, float* counts, float* totalcounts,
                  int* labels_out, void* workspace, hipStream_t s);
int launch_cosine_assign(const float* x, long N, int d, const float* cent, int k, int take_min, float* w32_scratch,
                         int* labels, float* sims, hipStream_t s);
// apply_r.lua:218-227: per cluster j < k the min(m, members) rows with the largest similarity (descending, ties by ascending row, NaN last) into
// rows_out / sims_out [k][m] (unused slots -1 / 0), kept_out [k] = rows written, sizes_out [k] = members.  All pointers device.  Returns 1
// outside k <= 32, m <= 128, 1 <= n < 2^31.
size_t cluster_members_workspace_bytes(long n, int k);
int launch_cluster_members(const int* labels, const float* sims, long n, int k, int m, long* rows_out, float* sims_out, int* kept_out, int* sizes_out,
                           void* workspace, hipStream_t s);
// gr_cluster_dev: apply_r.lua:198-227 in one enqueue, 1 <= k <= 4096, d <= 256, 1 <= m <= 128, 1 <= n < 2^31 (returns 1 outside, 2 when the device refuses
// the wide assignment kernel's LDS).  Below g_cluster_wide_min_k (and while k * d doubles fit kmeans_accumulate_kernel's 60 KB) the three launch_* above,
// in their order; from it on the wide kernels of kmeans.hip, which reproduce their bits.  c2 / counts / w32 / totalcounts [k] device scratch.
extern int g_cluster_wide_min_k;         // gr_set_tuning "cluster_wide_min_k" (default 33)
bool cluster_takes_wide_route(int d, int k);
size_t cluster_workspace_bytes(long n, int d, int k);
int launch_cluster(const float* x, long n, int d, int k, int niter, float* cent, int take_min, int m, float* c2, float* counts, float* totalcounts,
                   float* w32, int* labels, float* sims, long* rows_out, float* sims_out, int* kept_out, int* sizes_out, void* workspace, hipStream_t s);
// gr_cluster_members_wide_dev: launch_cluster_members' lists by the wide route's grouping and selection kernels (the helper launch_cluster uses), for
// 1 <= k <= 4096, 1 <= m <= 128, 1 <= n < 2^31 (returns 1 outside).
size_t cluster_members_wide_workspace_bytes(long n, int k);
int launch_cluster_members_wide(const int* labels, const float* sims, long n, int k, int m, long* rows_out, float* sims_out, int* kept_out, int* sizes_out,
                                void* workspace, hipStream_t s);
// The wide route's index of a labelling, for the callers outside kmeans.hip (silhouette.hip): wide_group_kernel sorts every block of 512 rows by
// (label, row) - order [blocks x 512], the rows with a label in [0, k) first - and lists the block's segments: seg_label / seg_start [block][segs]
// (ascending labels, first position in the block's order), nseg / nvalid [block].  wide_index_carve takes wide_index_bytes(n, k) from ws and moves
// ws past them; 1 <= k <= 4096, 1 <= n < 2^31.
struct WideIndex { int *seg_label, *seg_start, *nseg, *nvalid, *order; };
int wide_index_segs(int k);
size_t wide_index_bytes(long n, int k);
WideIndex wide_index_carve(char*& ws, long n, int k);
int wide_group(const int* labels, long n, int k, const WideIndex& ix, hipStream_t s);
// apply_r.lua:233-243 for every cluster at once: out[j] = launch_rows_mean of rows[j][0 .. kept[j]); entries outside [0, n_rows) are skipped
void launch_cluster_faces(const float* x, long n_rows, long d, const long* rows, const int* kept, int k, int m, float* out, hipStream_t s);

// ---------------------------------------------------------------- principal axes of a device table (pca.hip; gr_pca_dev, gr_pca_project_dev)
// mean [d] / cov [d][d] (nullable) / eigvals [d] doubles, axes [d][d] floats (row = unit axis), info [2] ints (sweeps, converged): all device;
// workspace from pca_workspace_bytes.  Returns 1 outside 2 <= n < 2^31, 1 <= d <= 256.
size_t pca_workspace_bytes(long n, int d);
int launch_pca(const float* x, long n, int d, double* mean, double* cov, double* eigvals, float* axes, int* info, void* workspace, hipStream_t s);
// out [n][k] = (x - mean) . axes[0 .. k)^T, column a times 1 / sqrt(eigvals[a]) when whiten (0 for eigvals[a] <= 0).  Returns 1 outside
// 1 <= n < 2^31, 1 <= k <= d <= 256, 2 when the device refuses the kernel's LDS.
int launch_pca_project(const float* x, long n, int d, const double* mean, const float* axes, const double* eigvals, int k, int whiten, float* out,
                       hipStream_t s);

// ---------------------------------------------------------------- diagonal Gaussian mixture of a device table (mixture.hip; gr_mixture_dev)
// niter x (E-step, M-step), then one E-step: w [k], mu / vars [k][d] floats in and out, loglik [niter + 1] doubles, labels / post / rowll [n] nullable:
// all device; workspace from mixture_workspace_bytes.  Returns 1 outside 1 <= n < 2^31, 1 <= d, k <= 256, niter >= 0, var_floor > 0, and 2 when the
// device refuses the kernels' LDS.
size_t mixture_workspace_bytes(long n, int d, int k);
int launch_mixture(const float* x, long n, int d, int k, int niter, float var_floor, float* w, float* mu, float* vars, double* loglik, int* labels,
                   float* post, float* rowll, void* workspace, hipStream_t s);

// ---------------------------------------------------------------- silhouette coefficients of a labelled device table (silhouette.hip; gr_silhouette_dev)
// x [n x d] floats, labels [n]; s [n], a / b / nearest [n] nullable, cluster_mean [k], sizes [k], mean 1 double: all device; workspace from
// silhouette_workspace_bytes.  metric 0 euclidean, 1 cosine.  Returns 1 outside 2 <= n <= SIL_MAX_N, 1 <= d <= 256, 1 <= k <= 4096, metric 0 / 1.
constexpr long SIL_MAX_N = 262144;
size_t silhouette_workspace_bytes(long n, int k);
int launch_silhouette(const float* x, long n, int d, const int* labels, int k, int metric, double* s_out, double* a_out, double* b_out, int* nearest,
                      double* cluster_mean, int* sizes, double* mean, void* workspace, hipStream_t s);

// ---------------------------------------------------------------- the k-nearest-neighbour graph of a device table (knn.hip; gr_knn_dev, gr_lof_dev, gr_knn_overlap_dev)
// x [n x d] floats; idx [n x k] ints, dist [n x k] doubles: row i's k nearest rows j != i by (dist, j) ascending, silhouette.hip's pair distances; lrd
// (nullable) / lof [n] doubles; count [n] ints, mean 1 double: all device; workspaces from the *_workspace_bytes beside each.  metric 0 euclidean, 1
// cosine.  All return 1 outside 2 <= n <= KNN_MAX_N, 1 <= k <= min(n - 1, 128), and launch_knn outside 1 <= d <= 256, metric 0 / 1 too.
constexpr long KNN_MAX_N = SIL_MAX_N;
size_t knn_workspace_bytes(long n);
int launch_knn(const float* x, long n, int d, int k, int metric, int* idx_out, double* dist_out, void* workspace, hipStream_t s);
size_t lof_workspace_bytes(long n);
int launch_lof(const int* idx, const double* dist, long n, int k, double* lrd, double* lof, void* workspace, hipStream_t s);
size_t knn_overlap_workspace_bytes(long n);
int launch_knn_overlap(const int* a, const int* b, long n, int k, int* count, double* mean, void* workspace, hipStream_t s);

// ---------------------------------------------------------------- density-based clustering of a device table (density.hip; gr_eps_graph_dev, gr_dbscan_dev)
// x [n x d] floats; adj [n x ceil(n / 64)] 64-bit words: bit j of row i set iff silhouette.hip's pair distance of (i, j) is <= eps, or j = i; count
// [n] ints: the rows' popcounts; labels / core (nullable) [n] ints, n_clusters 1 int: all device.  metric 0 euclidean, 1 cosine.  launch_eps_graph
// returns 1 outside 2 <= n <= DBSCAN_MAX_N, 1 <= d <= 256, eps finite and >= 0, metric 0 / 1; launch_dbscan_begin outside that n or 1 <= min_pts <= n.
// gr_dbscan_dev's three parts share a carved workspace of dbscan_workspace_bytes: begin (core flags, label = the row itself), then the caller repeats
// round (one hook-and-compress pass; *w.changed is 1 afterwards where a label fell) until one changes nothing, then finish (border rows, cluster
// numbers).  n rounds always suffice.
constexpr long DBSCAN_MAX_N = SIL_MAX_N;
struct DbscanScratch { int* label; int* rank; int* changed; unsigned long long* mask; };
size_t eps_graph_workspace_bytes(long n);
int launch_eps_graph(const float* x, long n, int d, double eps, int metric, unsigned long long* adj, int* count, void* workspace, hipStream_t s);
size_t dbscan_workspace_bytes(long n);
DbscanScratch dbscan_carve(void* workspace, long n);
int launch_dbscan_begin(const int* count, long n, int min_pts, const DbscanScratch& w, hipStream_t s);
void launch_dbscan_round(const unsigned long long* adj, long n, const DbscanScratch& w, hipStream_t s);
void launch_dbscan_finish(const unsigned long long* adj, long n, const DbscanScratch& w, int* labels, int* core, int* n_clusters, hipStream_t s);

// ---------------------------------------------------------------- the minimum spanning tree of a device table (mst.hip; gr_mst_dev)
// x [n x d] floats; core (nullable) doubles, row i's at core[i * core_stride]; eu / ev [n - 1] ints, ew [n - 1] doubles: all device.  The weight of
// the pair (i, j) is silhouette.hip's pair distance, raised to core_i and core_j where they are larger; the tree is the unique one under the order
// (w, min(i, j), max(i, j)).  launch_mst_begin returns 1 outside 2 <= n <= MST_MAX_N, 1 <= d <= 256, metric 0 / 1.  The three parts share a carved
// workspace of mst_workspace_bytes: begin (norms, comp[i] = i, *w.n_edges = 0), then the caller repeats round (every component's smallest outgoing
// edge, hook, compress; *w.n_edges counts the edges emitted so far) until n - 1 edges are out - ceil(log2 n) rounds always suffice - then finish (the
// edges to eu / ev / ew in the edge order).
constexpr long MST_MAX_N = SIL_MAX_N;
struct MstScratch {
  double* qn; double* best_w; unsigned long long* cw; unsigned long long* ce; unsigned long long* edge_w; unsigned long long* edge_e;
  int* comp; int* parent; int* best_j; int* n_edges;
};
size_t mst_workspace_bytes(long n);
MstScratch mst_carve(void* workspace, long n);
int launch_mst_begin(const float* x, long n, int d, int metric, const MstScratch& w, hipStream_t s);
void launch_mst_round(const float* x, long n, int d, int metric, const double* core, long core_stride, const MstScratch& w, hipStream_t s);
void launch_mst_finish(long n, const MstScratch& w, int* eu, int* ev, double* ew, hipStream_t s);

// ---------------------------------------------------------------- the sampling layer of a VAE (vae.hip; gr_vae_sample_dev, gr_vae_sample_backward_dev)
// h [B x 2 nd] = (mu | logvar), eps (nullable: 0) / z / gz [B x nd], gh [B x 2 nd], kl_rows [B] floats and kl 1 double nullable: all device; workspace
// of chain_mean_workspace_bytes(B), read only when kl is given; c = kl_weight / B.  Both return 1 outside 1 <= B < 2^31, 1 <= nd <= 256.
int launch_vae_sample(const float* h, const float* eps, long B, int nd, float* z, float* kl_rows, double* kl, void* workspace, hipStream_t s);
int launch_vae_sample_backward(const float* h, const float* eps, const float* gz, long B, int nd, double c, float* gh, hipStream_t s);

// ---------------------------------------------------------------- SSIM and MSE per image (quality.hip; gr_ssim_dev)
// a, b [n x channels x h x w], ssim_rows [n], mse_rows [n] nullable, mean 1 double nullable: all device; workspace of chain_mean_workspace_bytes(n), read only
// when mean is given.  sigma <= 0: the uniform window.  Returns 1 outside the limits of ssim_args_ok or for a data_range that is not > 0, and 2 when
// the device refuses the kernel's LDS.
bool ssim_args_ok(long n, int channels, int h, int w, int win);
int launch_ssim(const float* a, const float* b, long n, int channels, int h, int w, int win, double sigma, double data_range, float* ssim_rows, float* mse_rows,
                double* mean, void* workspace, hipStream_t s);

// ---------------------------------------------------------------- exact t-SNE of a device table (tsne.hip; gr_tsne_*_dev, gr_map_cells_dev)
// Every pointer is device memory.  The launchers return 1 outside their limits (n <= 16384; affinities n >= 4, d >= 1; cells: grid sides 1 .. 1024),
// launch_tsne_affinities 2 when the device refuses a memset.  One workspace of tsne_iter_workspace_bytes serves gradient, KL and update.
size_t tsne_affinities_workspace_bytes(int n, int d);
size_t tsne_iter_workspace_bytes(int n);
size_t map_cells_workspace_bytes(int cells);
int launch_tsne_affinities(const float* x, int n, int d, double perplexity, float* p, double* beta /*nullable*/, int* info, void* workspace, hipStream_t s);
int launch_tsne_gradient(const float* p, const float* y, int n, float exaggeration, float* grad, double* z /*nullable*/, void* workspace, hipStream_t s);
int launch_tsne_kl(const float* p, const float* y, int n, double* kl, void* workspace, hipStream_t s);
int launch_tsne_update(float* y, const float* grad, float* inc, float* gains, int n, float eta, float momentum, float min_gain, void* workspace,
                       hipStream_t s);
int launch_map_cells(const float* y, long n, int gh, int gw, long* rows_out, int* counts /*nullable*/, void* workspace, hipStream_t s);

// mfmaloop.hip: the bare LDS-read + f16x3 MFMA loop (sustained ceiling of the convolution inner loop on this device; diagnostic)
size_t mfma_loop_workspace_bytes();
double mfma_loop_flops(int iters);
void launch_mfma_loop_fill(void* workspace, hipStream_t s);
void launch_mfma_loop(int shape, void* workspace, int iters, hipStream_t s);
}  // namespace gr
