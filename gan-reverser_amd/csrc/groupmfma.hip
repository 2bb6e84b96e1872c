// groupmfma.hip — GR_GROUPCONV3 (group.hip) on the matrix cores in the split arithmetics of DESIGN.md section 3: f16x3 (two fp16 terms, the
// products x0w0, x0w1, x1w0) and bf16x6 (three bf16 terms, the six products of order < 3, no scaling), v_mfma_f32_16x16x32_f16 / _bf16 with
// fp32 accumulation.  Same contract as group.hip's launches: fp32 NCHW on both sides, weight [Cout][Cin/G][3][3] read as it is, `up` indexes
// the half-size input in place, gw +=.  There is no weight image, no operand-ready tensor and no scale slot: every operand is split while it
// is staged (global fp32 -> registers -> split -> LDS or MFMA fragment).
//
// SHAPE (groupconv3_mfma_supported): exactly 16 input and 16 output planes per group, planes of H <= 32 and W <= 32 (even when `up`), any B
// and G - create_G4's grouped convolution.  One (image, group) tile then fits LDS whole; everything else stays on group.hip's fp32 kernels.
//
// f16x3 SCALE: one power of two per (image, group) activation / gradOutput tile and one per group for its 2304 weights, measured by the
// workgroup that stages them (f16_scale_exp of the tile's max|.|; a tile of zeros takes 2^0).  The scale-back is one exact ldexp.  So an
// image's result does not depend on the batch around it, and these stages neither trip nor consult the range guard.  Weight-gradient
// accumulators of two images carry different scales: they are scaled back per image and added into fp32 sums, never inside the MFMA.
//
// ORDER: no float atomics; every sum has a fixed order (the MFMA chain of a tile, the four waves in index order, images in index order,
// the splits' partials in split order by group.hip's group_wgrad_reduce_kernel): two runs give the same bits.
//
// forward / data gradient (one kernel, template DGRAD): workgroup = one (image, group), 256 threads.  LDS: the zero-padded input planes,
// channels last - [term][(H + 2) x (W + 2) cells][16 planes] - so the 8 consecutive k of an A fragment (k = 16 tap + plane) are one 16-byte
// read.  D[pixel][plane]: M = 16 pixels per tile, N = 16 planes, K = 144 padded to 160 (a tenth tap of zeros), five MFMA steps per product.
// The B fragments (weights; the data gradient reads them transposed and flipped) are split once into registers.  A lane ends with 4
// consecutive pixels of one plane: a 16-byte store.  Behind an up-sampling the forward writes each source pixel to its four cells; the data
// gradient's tiles are 4 source pixels x their 2 x 2 block, and a lane adds its four accumulators ((d00 + d01) + d10) + d11.
//
// weight gradient: workgroup = (group, split of the batch), its images one after another.  K = pixels in a row pitch P = round_up(W + 2, 8):
// k = y P + x.  LDS: the zero-padded input planes, plane-major [term][16][k], so the B fragment of tap (ky, kx) is the 8 halves from
// k + ky P + kx on: one aligned 16-byte + one 4-byte read per (term, ky), shifted in registers by kx halves.  The A fragment (gradOutput,
// 8 consecutive pixels of a row, zero where x >= W) comes straight from global memory and serves all nine taps.  Wave w takes the 32-k steps
// w, w + 4, ...; the waves' 9 x 16 x 16 accumulators meet in LDS (over the planes, which are staged anew per image).
#include "kernels.h"

namespace gr {

int g_group_mfma_min_tiles = 512;      // gr_set_tuning "group_mfma_min_tiles": the MFMA launches run from this many (image, group) tiles on

typedef short gm_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int GM_PLANES = 16;          // input and output planes per group
constexpr int GM_MAX_HW = 32;          // largest plane side
constexpr int GM_KSTEPS = 5;           // MFMA steps of the forward / data gradient: 9 taps x 16 planes = 144, padded to 160 = 5 x 32
constexpr int GM_MAX_SPLITS = 16;      // batch splits of the weight gradient (= group.hip's GC_MAX_SPLITS: groupconv3_workspace_bytes holds the partials)
constexpr int GM_RED_FLOATS = 4 * 9 * 256;     // the weight gradient's cross-wave scratch: 4 waves x 9 taps x 16 x 16

bool groupconv3_mfma_supported(int Cin, int Cout, int G, int H, int W, bool up) {
  return G >= 1 && Cin == GM_PLANES * G && Cout == GM_PLANES * G && H >= 1 && H <= GM_MAX_HW && W >= 1 && W <= GM_MAX_HW && (!up || (H % 2 == 0 && W % 2 == 0));
}

// 8 floats (times sc) -> NTERM vectors of 8 fp16 / bf16 terms, round-to-nearest each time; every remainder is exact in fp32
template <int NTERM>
__device__ __forceinline__ void gm_split8(const float* x, float sc, uint4 (&t)[NTERM]) {
  unsigned short h[NTERM][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float r = NTERM == 2 ? x[j] * sc : x[j];
#pragma unroll
    for (int i = 0; i < NTERM; ++i) {
      if (NTERM == 2) { const _Float16 v = (_Float16)r; h[i][j] = __builtin_bit_cast(unsigned short, v); r -= (float)v; }
      else { const __bf16 v = (__bf16)r; h[i][j] = __builtin_bit_cast(unsigned short, v); r -= __uint_as_float((unsigned)h[i][j] << 16); }
    }
  }
#pragma unroll
  for (int i = 0; i < NTERM; ++i)
    t[i] = make_uint4(h[i][0] | (unsigned)h[i][1] << 16, h[i][2] | (unsigned)h[i][3] << 16, h[i][4] | (unsigned)h[i][5] << 16, h[i][6] | (unsigned)h[i][7] << 16);
}
template <int NTERM>
__device__ __forceinline__ f32x4 gm_mma(const uint4& a, const uint4& b, f32x4 c) {
  if (NTERM == 2) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gm_bf16x8, a), __builtin_bit_cast(gm_bf16x8, b), c, 0, 0, 0);
}
// the products kept, smallest first, as (A term, B term): f16x3 (1,0) (0,1) (0,0); bf16x6 (2,0) (1,1) (0,2) (1,0) (0,1) (0,0)
template <int NTERM> __host__ __device__ constexpr int gm_nprod() { return NTERM == 2 ? 3 : 6; }
template <int NTERM> __host__ __device__ constexpr int gm_prod_a(int pr) { return NTERM == 2 ? (pr == 0 ? 1 : 0) : (pr == 0 ? 2 : (pr == 1 || pr == 3) ? 1 : 0); }
template <int NTERM> __host__ __device__ constexpr int gm_prod_b(int pr) { return NTERM == 2 ? (pr == 1 ? 1 : 0) : (pr == 2 ? 2 : (pr == 1 || pr == 4) ? 1 : 0); }

// max over the workgroup's 256 threads of bit patterns of |.| (order-free); sh: 4 words
__device__ __forceinline__ unsigned gm_block_max(unsigned v, unsigned* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  __syncthreads();                                  // (sh may still be read by the previous call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}
__device__ __forceinline__ unsigned gm_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

struct GmArgs {
  const float* in; const float* w; const float* bias; float* out;
  int G, H, W, up, vec;            // H x W: the convolution's planes; vec: 16-byte stores are aligned
};

// forward:        out[bi][g 16 + n][p] = bias + sum_{tap, c} in[bi][g 16 + c][p + tap] W[g 16 + n][c][tap]           (in: H/2 x W/2 planes when up)
// data gradient:  gin[bi][g 16 + n][p] = sum_{tap, c} gout[bi][g 16 + c][p + tap] W[g 16 + c][n][8 - tap]          (a.in = gout, a.out = gin;
//                 up: gin's planes are H/2 x W/2 and an element is the sum over its 2 x 2 block of p)
// grid (G, B)
template <int NTERM, int DGRAD>
__global__ __launch_bounds__(256) void groupconv3_mfma_conv_kernel(GmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gm_smem[];
  __shared__ unsigned shmax[8];
  uint4* cellv = reinterpret_cast<uint4*>(gm_smem);           // [NTERM][cells][2 halves of 8 planes]
  const int g = blockIdx.x, bi = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int H = a.H, W = a.W, HW = H * W, PW = W + 2, cells = (H + 2) * PW;
  const int up_in = DGRAD ? 0 : a.up, up_out = DGRAD ? a.up : 0;
  const int Hs = up_in ? H >> 1 : H, Ws = up_in ? W >> 1 : W, HWs = Hs * Ws;          // the planes staged
  const int Ho = up_out ? H >> 1 : H, Wo = up_out ? W >> 1 : W, HWo = Ho * Wo;        // the planes written
  const int C = GM_PLANES * a.G;
  const float* inb = a.in + ((long)bi * C + (long)g * GM_PLANES) * HWs;               // the tile: 16 consecutive planes
  const float* wg = a.w + (long)g * GM_PLANES * GM_PLANES * 9;
  int kx_ = 0, kw_ = 0;
  if (NTERM == 2) {
    unsigned mx = 0, mw = 0;
    for (int i = tid; i < GM_PLANES * HWs; i += 256) mx = max(mx, gm_absbits(inb[i]));
    for (int i = tid; i < GM_PLANES * GM_PLANES * 9; i += 256) mw = max(mw, gm_absbits(wg[i]));
    kx_ = f16_scale_exp(gm_block_max(mx, shmax));
    kw_ = f16_scale_exp(gm_block_max(mw, shmax + 4));
  }
  const float sc_x = pow2f(kx_), sc_w = pow2f(kw_);
  // the zero border
  for (int c = tid; c < cells; c += 256) {
    const int yy = c / PW, xx = c - yy * PW;
    if (yy == 0 || yy == H + 1 || xx == 0 || xx == W + 1) {
#pragma unroll
      for (int t = 0; t < NTERM; ++t) { cellv[(t * cells + c) * 2] = make_uint4(0, 0, 0, 0); cellv[(t * cells + c) * 2 + 1] = make_uint4(0, 0, 0, 0); }
    }
  }
  // the planes: (source pixel, 8-plane half) per thread
  for (int i = tid; i < 2 * HWs; i += 256) {
    const int h = i >= HWs ? 1 : 0, sp = i - h * HWs;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = inb[(long)(8 * h + j) * HWs + sp];
    uint4 t[NTERM];
    gm_split8<NTERM>(v, sc_x, t);
    const int ys = sp / Ws, xs = sp - ys * Ws;
    if (up_in) {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int c = (2 * ys + (d >> 1) + 1) * PW + 2 * xs + (d & 1) + 1;
#pragma unroll
        for (int tt = 0; tt < NTERM; ++tt) cellv[(tt * cells + c) * 2 + h] = t[tt];
      }
    } else {
      const int c = (ys + 1) * PW + xs + 1;
#pragma unroll
      for (int tt = 0; tt < NTERM; ++tt) cellv[(tt * cells + c) * 2 + h] = t[tt];
    }
  }
  // B fragments: lane (n, q) of step s holds k = 32 s + 8 q + j: tap 2 s + (q >> 1), planes 8 (q & 1) + j; tap 9 is the padding
  uint4 bw[GM_KSTEPS][NTERM];
#pragma unroll
  for (int s = 0; s < GM_KSTEPS; ++s) {
    const int tap = 2 * s + (q >> 1), c0 = 8 * (q & 1);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      v[j] = tap < 9 ? (DGRAD ? wg[(c * GM_PLANES + n) * 9 + 8 - tap] : wg[(n * GM_PLANES + c) * 9 + tap]) : 0.f;
    }
    gm_split8<NTERM>(v, sc_w, bw[s]);
  }
  __syncthreads();
  const int ntiles = up_out ? (HWo + 3) / 4 : (HW + 15) / 16;
  const float bv = DGRAD ? 0.f : a.bias[g * GM_PLANES + n];
  float* outb = a.out + ((long)bi * C + (long)g * GM_PLANES + n) * HWo;
  for (int t0 = 2 * wave; t0 < ntiles; t0 += 8) {               // two tiles per round: two independent MFMA chains
    int base[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = t0 + u, m = lane & 15;
      int y, x;
      if (up_out) {
        const int sp = 4 * tile + (m >> 2), spc = sp < HWo ? sp : 0, ys = spc / Wo, xs = spc - ys * Wo;
        y = 2 * ys + ((m >> 1) & 1); x = 2 * xs + (m & 1);
      } else {
        const int p = 16 * tile + m, pc = p < HW ? p : 0;
        y = pc / W; x = pc - y * W;
      }
      base[u] = y * PW + x;
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < GM_KSTEPS; ++s) {
      const int tap = 2 * s + (q >> 1), tc = tap < 9 ? tap : 8, off = (tc / 3) * PW + tc % 3;
      uint4 av[2][NTERM];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
          av[u][t] = cellv[(t * cells + base[u] + off) * 2 + (q & 1)];
          if (s == GM_KSTEPS - 1 && tap >= 9) av[u][t] = make_uint4(0, 0, 0, 0);
        }
#pragma unroll
      for (int pr = 0; pr < gm_nprod<NTERM>(); ++pr)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[u] = gm_mma<NTERM>(av[u][gm_prod_a<NTERM>(pr)], bw[s][gm_prod_b<NTERM>(pr)], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int tile = t0 + u;
      if (tile >= ntiles) continue;
      if (up_out) {
        const int sp = 4 * tile + q;
        const float v = ((acc[u][0] + acc[u][1]) + acc[u][2]) + acc[u][3];
        if (sp < HWo) outb[sp] = NTERM == 2 ? ldexpf(v, -(kx_ + kw_)) : v;
      } else {
        const int p = 16 * tile + 4 * q;
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (NTERM == 2 ? ldexpf(acc[u][e], -(kx_ + kw_)) : acc[u][e]) + bv;
        if (a.vec) { if (p < HW) *reinterpret_cast<float4*>(outb + p) = make_float4(r[0], r[1], r[2], r[3]); }
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (p + e < HW) outb[p + e] = r[e];
        }
      }
    }
  }
}

struct GmWgradArgs {
  const float* in; const float* gout; float* part;
  int B, G, H, W, up, per_split, P, ksteps, PL;     // P: row pitch of k; ksteps = ceil(H P / 32); PL: halves of one LDS plane
};
// part[split][g 16 + oc][ci][tap] = sum over the split's images, in order, of sum_p gout[bi][g 16 + oc][p] in[bi][g 16 + ci][p + tap]
// grid (G, splits)
template <int NTERM>
__global__ __launch_bounds__(256) void groupconv3_mfma_wgrad_kernel(GmWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gm_smem[];
  __shared__ unsigned shmax[8];
  unsigned short* xl = reinterpret_cast<unsigned short*>(gm_smem);      // [NTERM][16][PL]
  float* red = reinterpret_cast<float*>(gm_smem);                       // [4 waves][9][4][64], over the planes once they are consumed
  const int g = blockIdx.x, split = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int H = a.H, W = a.W, HW = H * W, P = a.P, PL = a.PL;
  const int Hs = a.up ? H >> 1 : H, Ws = a.up ? W >> 1 : W, HWs = Hs * Ws;
  const int C = GM_PLANES * a.G;
  const int bbeg = split * a.per_split, bend = min(a.B, bbeg + a.per_split);
  const int nzero = NTERM * GM_PLANES * PL / 8;                         // uint4s of the planes (PL % 8 == 0)
  float sum[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) sum[i] = 0.f;
  for (int bi = bbeg; bi < bend; ++bi) {
    const float* xb = a.in + ((long)bi * C + (long)g * GM_PLANES) * HWs;
    const float* gb = a.gout + ((long)bi * C + (long)g * GM_PLANES) * HW;
    int kx_ = 0, kg_ = 0;
    if (NTERM == 2) {
      unsigned mx = 0, mg = 0;
      for (int i = tid; i < GM_PLANES * HWs; i += 256) mx = max(mx, gm_absbits(xb[i]));
      for (int i = tid; i < GM_PLANES * HW; i += 256) mg = max(mg, gm_absbits(gb[i]));
      kx_ = f16_scale_exp(gm_block_max(mx, shmax));
      kg_ = f16_scale_exp(gm_block_max(mg, shmax + 4));
    }
    const float sc_x = pow2f(kx_), sc_g = pow2f(kg_);
    __syncthreads();                                                    // the previous image's scratch has been read
    for (int i = tid; i < nzero; i += 256) reinterpret_cast<uint4*>(gm_smem)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    // plane ci, pixel (y, x) -> k = (y + 1) P + x + 1
    for (int i = tid; i < GM_PLANES * HWs; i += 256) {
      const int ci = i / HWs, sp = i - ci * HWs, ys = sp / Ws, xs = sp - ys * Ws;
      float r = NTERM == 2 ? xb[i] * sc_x : xb[i];
      unsigned short h[NTERM];
#pragma unroll
      for (int t = 0; t < NTERM; ++t) {
        if (NTERM == 2) { const _Float16 v = (_Float16)r; h[t] = __builtin_bit_cast(unsigned short, v); r -= (float)v; }
        else { const __bf16 v = (__bf16)r; h[t] = __builtin_bit_cast(unsigned short, v); r -= __uint_as_float((unsigned)h[t] << 16); }
      }
#pragma unroll
      for (int t = 0; t < NTERM; ++t) {
        unsigned short* pl = xl + (t * GM_PLANES + ci) * PL;
        if (a.up) {
          const int k = (2 * ys + 1) * P + 2 * xs + 1;
          pl[k] = h[t]; pl[k + 1] = h[t]; pl[k + P] = h[t]; pl[k + P + 1] = h[t];
        } else pl[(ys + 1) * P + xs + 1] = h[t];
      }
    }
    __syncthreads();
    f32x4 acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int step = wave; step < a.ksteps; step += 4) {
      const int k0 = step * 32 + 8 * q, y = k0 / P, x0 = k0 - y * P;
      // A: gradOutput plane n, pixels (y, x0 .. x0 + 7), zero outside the plane
      float v[8];
      const float* gp = gb + (long)n * HW + y * W + x0;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (y < H && x0 + j < W) ? gp[j] : 0.f;
      uint4 at[NTERM];
      gm_split8<NTERM>(v, sc_g, at);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        uint4 bt[3][NTERM];                                              // [kx][term]
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
          const int hb = (t * GM_PLANES + n) * PL + k0 + ky * P;         // % 8 == 0
          const uint4 d = *reinterpret_cast<const uint4*>(xl + hb);
          const unsigned d4 = *reinterpret_cast<const unsigned*>(xl + hb + 8);
          bt[0][t] = d;
          bt[1][t] = make_uint4(d.x >> 16 | d.y << 16, d.y >> 16 | d.z << 16, d.z >> 16 | d.w << 16, d.w >> 16 | d4 << 16);
          bt[2][t] = make_uint4(d.y, d.z, d.w, d4);
        }
#pragma unroll
        for (int pr = 0; pr < gm_nprod<NTERM>(); ++pr)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
            acc[ky * 3 + kx] = gm_mma<NTERM>(at[gm_prod_a<NTERM>(pr)], bt[kx][gm_prod_b<NTERM>(pr)], acc[ky * 3 + kx]);
      }
    }
    __syncthreads();                                                    // every wave is done with the planes
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave * (9 * 256) + (i * 4 + r) * 64 + lane] = acc[i][r];
    __syncthreads();
    // thread tid owns (tap i, row 4 (lane >> 4) + (tid >> 6), column lane & 15): the four waves in order, scaled back, onto the images before
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const float s = ((red[i * 256 + tid] + red[9 * 256 + i * 256 + tid]) + red[2 * 9 * 256 + i * 256 + tid]) + red[3 * 9 * 256 + i * 256 + tid];
      sum[i] += NTERM == 2 ? ldexpf(s, -(kx_ + kg_)) : s;
    }
  }
  const int oc = 4 * q + wave, ci = n;
#pragma unroll
  for (int i = 0; i < 9; ++i) a.part[(((long)split * C + g * GM_PLANES + oc) * GM_PLANES + ci) * 9 + i] = sum[i];
}

static double gm_flops(int B, int G, int H, int W) { return 2.0 * B * H * W * (double)GM_PLANES * G * GM_PLANES * 9; }
static double gm_bytes(int B, int G, int H, int W, bool up) { return 4.0 * B * GM_PLANES * G * ((double)H * W / (up ? 4 : 1) + (double)H * W); }
static size_t gm_conv_lds(int nterm, int H, int W) { return (size_t)nterm * (H + 2) * (W + 2) * 32; }
template <int NTERM, int DGRAD>
static void gm_launch_conv(const GmArgs& a, int B, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&groupconv3_mfma_conv_kernel<NTERM, DGRAD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)gm_conv_lds(NTERM, GM_MAX_HW, GM_MAX_HW));
    attr = true;
  }
  groupconv3_mfma_conv_kernel<NTERM, DGRAD><<<dim3((unsigned)a.G, (unsigned)B), 256, gm_conv_lds(NTERM, a.H, a.W), s>>>(a);
}
static bool gm_vec_ok(const float* out, int HW) { return HW % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0; }

// mode: 2 = f16x3, anything else = bf16x6 (the context's GR_CONV_MODE; f32 never comes here)
void launch_groupconv3_mfma_forward(const float* in, const float* w, const float* bias, float* out, int B, int G, int H, int W, bool up, int mode, hipStream_t s) {
  KtScope kt("groupconv3_mfma_forward_kernel", gm_flops(B, G, H, W), gm_bytes(B, G, H, W, up), s);
  const GmArgs a{in, w, bias, out, G, H, W, up ? 1 : 0, gm_vec_ok(out, H * W) ? 1 : 0};
  if (mode == 2) gm_launch_conv<2, 0>(a, B, s); else gm_launch_conv<3, 0>(a, B, s);
}
void launch_groupconv3_mfma_backward_data(const float* gout, const float* w, float* gin, int B, int G, int H, int W, bool up, int mode, hipStream_t s) {
  KtScope kt("groupconv3_mfma_dgrad_kernel", gm_flops(B, G, H, W), gm_bytes(B, G, H, W, up), s);
  const GmArgs a{gout, w, nullptr, gin, G, H, W, up ? 1 : 0, (!up && gm_vec_ok(gin, H * W)) ? 1 : 0};
  if (mode == 2) gm_launch_conv<2, 1>(a, B, s); else gm_launch_conv<3, 1>(a, B, s);
}

static int gm_splits(int B) { return B < GM_MAX_SPLITS ? B : GM_MAX_SPLITS; }
template <int NTERM>
static void gm_launch_wgrad(const GmWgradArgs& a, int used, hipStream_t s) {
  const int pmax = round_up(GM_MAX_HW + 2, 8), plmax = round_up(GM_MAX_HW * pmax, 32) + 2 * pmax + 16;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&groupconv3_mfma_wgrad_kernel<NTERM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((size_t)NTERM * GM_PLANES * plmax * 2));
    attr = true;
  }
  size_t lds = (size_t)NTERM * GM_PLANES * a.PL * 2;
  if (lds < sizeof(float) * GM_RED_FLOATS) lds = sizeof(float) * GM_RED_FLOATS;
  groupconv3_mfma_wgrad_kernel<NTERM><<<dim3((unsigned)a.G, (unsigned)used), 256, lds, s>>>(a);
}
// ws: groupconv3_workspace_bytes(B, 16 G, 16 G, G)
void launch_groupconv3_mfma_backward_weight(const float* in, const float* gout, float* gw, void* ws, int B, int G, int H, int W, bool up, int mode, hipStream_t s) {
  const int splits = gm_splits(B), per = (B + splits - 1) / splits, used = (B + per - 1) / per;      // every split owns at least one image
  const int P = round_up(W + 2, 8), ksteps = (H * P + 31) / 32;
  float* part = static_cast<float*>(ws);
  {
    KtScope kt("groupconv3_mfma_wgrad_kernel", gm_flops(B, G, H, W), gm_bytes(B, G, H, W, up), s);
    const GmWgradArgs a{in, gout, part, B, G, H, W, up ? 1 : 0, per, P, ksteps, ksteps * 32 + 2 * P + 16};
    if (mode == 2) gm_launch_wgrad<2>(a, used, s); else gm_launch_wgrad<3>(a, used, s);
  }
  const long n = (long)GM_PLANES * G * GM_PLANES * 9;
  KtScope kt("group_wgrad_reduce_kernel", (double)n * used, 4.0 * n * (used + 2), s);
  group_wgrad_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(part, gw, n, used);
}

}  // namespace gr
