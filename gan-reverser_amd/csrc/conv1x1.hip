// conv1x1.hip — nn.SpatialConvolution(Cin, Cout, 1, 1, 1, 1, 0, 0) on NCHW fp32: the pointwise convolutions of models.createResidual
// (reference models.lua:8-55; the bottleneck in front of and behind the two 3x3 layers, and the shortcut's reducer).
//
// A pointwise convolution is a GEMM whose long axis is the pixels of the whole batch: with n = b * HW + p,
//   forward          y[n][o]  = bias[o] + sum_i w[o][i] x[n][i]          M = Cout, K = Cin
//   data gradient    gin[n][i] =          sum_o w[o][i] gout[n][o]       M = Cin,  K = Cout   (the same kernel on the transposed weight)
//   weight gradient  gw[o][i] +=          sum_n gout[n][o] x[n][i]       a 64 x 64 tile, the reduction over n split over workgroups
// all three on v_mfma_f32_32x32x2_f32 with fp32 accumulation (exact fp32 in every GR_CONV_MODE, like convk.hip: no arithmetic modes).
// Element (n, c) of an NCHW tensor with C planes sits at (b * C + c) * HW + p: pixels are the contiguous axis, and a tile of
// consecutive n may cross image boundaries (HW smaller than a tile, or not a multiple of it) - every thread derives (b, p) of the
// pixels it stages once.  When HW % 4 == 0 and the tensors are 16-byte aligned four consecutive n lie in one image at an aligned
// address, and the staging loads are 16 bytes; otherwise they are scalar.
//   * forward / data gradient: a workgroup owns 128 pixels x 32 MB channels (MB = 1, 2 or 4: Cout <= 64 reads x once); wave w owns
//     pixels 32 w .. 32 w + 31 and every channel block.  Operands go through LDS in chunks of 32 reduction channels, the next chunk
//     is fetched into registers while the MFMAs of this one run (gemm.hip, gemm_mfma_kernel).  Pixels ride on the MFMA's column
//     (lane) axis, so one accumulator register of a wave is 32 consecutive pixels of one output plane: 128-byte row pieces per store.
//   * weight gradient: gemm_mfma_kernel's 64 x 64 tile with both operands pixel-contiguous; the n range is split into up to 512
//     slabs, summed in split order by a second launch and added (+=) into the gradient.  No atomics: two runs give the same bits.
// The bias gradient is not computed here: like every stage's, it comes from the pipeline backward (elem.hip, partials_b).
#include "kernels.h"

namespace gr {

typedef float c1_f32x16 __attribute__((ext_vector_type(16)));

constexpr int C1_NT = 128;        // pixels per workgroup (forward / data gradient)
constexpr int C1_KC = 32;         // reduction channels per LDS chunk

struct C1Args {
  const float* x; const float* w; const float* bias; float* y;
  int N, HW, K, M;                // N = B * HW pixels; K planes in, M planes out
  long wsm, wsk;                  // weight element (m, k) = w[m * wsm + k * wsk]
};

// MB: 32-channel blocks of the output per workgroup.  WK: the weight is contiguous along k (forward) or along m (data gradient).
template <int MB, bool WK>
__global__ __launch_bounds__(256) void conv1x1_kernel(C1Args a) {
  constexpr int MT = 32 * MB, WS = MT + 1, NW = 4 * MB;
  __shared__ __attribute__((aligned(16))) float Xs[C1_KC * C1_NT];
  __shared__ float Ws[C1_KC * WS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.x * C1_NT, m0 = blockIdx.y * MT;
  const bool vec = (a.HW & 3) == 0 && ((uintptr_t)a.x & 15) == 0;
  // the pixel(s) this thread stages: 4 consecutive ones x 4 channels (k = sk + 8 i), or one x 16 channels (k = sk + 2 i)
  const int spl = vec ? (tid & 31) * 4 : (tid & 127), sk = vec ? tid >> 5 : tid >> 7;
  const int sn = n0 + spl;
  const bool s_in = sn < a.N;       // (vec: N % 4 == 0, so the whole vector is inside)
  const int sb = s_in ? sn / a.HW : 0, sp = s_in ? sn - sb * a.HW : 0;
  const float* xp = a.x + (long)sb * a.K * a.HW + sp;
  float xv[16], wv[NW];
  auto load = [&](int k0) {
    if (vec) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + sk + 8 * i;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s_in && k < a.K) t = *reinterpret_cast<const float4*>(xp + (long)k * a.HW);
        xv[4 * i] = t.x; xv[4 * i + 1] = t.y; xv[4 * i + 2] = t.z; xv[4 * i + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = k0 + sk + 2 * i;
        xv[i] = (s_in && k < a.K) ? xp[(long)k * a.HW] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int f = tid + 256 * i, k = WK ? f & 31 : f / MT, m = WK ? f >> 5 : f % MT;
      wv[i] = (m0 + m < a.M && k0 + k < a.K) ? a.w[(long)(m0 + m) * a.wsm + (long)(k0 + k) * a.wsk] : 0.f;
    }
  };
  auto store = [&]() {
    if (vec) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(&Xs[(sk + 8 * i) * C1_NT + spl]) = make_float4(xv[4 * i], xv[4 * i + 1], xv[4 * i + 2], xv[4 * i + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) Xs[(sk + 2 * i) * C1_NT + spl] = xv[i];
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int f = tid + 256 * i, k = WK ? f & 31 : f / MT, m = WK ? f >> 5 : f % MT;
      Ws[k * WS + m] = wv[i];
    }
  };
  c1_f32x16 acc[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
  load(0);
  for (int k0 = 0; k0 < a.K; k0 += C1_KC) {
    store();
    __syncthreads();
    if (k0 + C1_KC < a.K) load(k0 + C1_KC);
    const int kn = min(C1_KC, (a.K - k0 + 1) & ~1);       // rows past K are zero in both operands: skip whole k pairs of them
    for (int kk = 0; kk < kn; kk += 2) {
      const float xq = Xs[(kk + h) * C1_NT + wave * 32 + l31];
#pragma unroll
      for (int b = 0; b < MB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[(kk + h) * WS + b * 32 + l31], xq, acc[b], 0, 0, 0);
    }
    __syncthreads();
  }
  // accumulator register r of block b: plane m0 + 32 b + 4 h + (r & 3) + 8 (r >> 2), pixel n0 + 32 wave + l31
  const int on = n0 + wave * 32 + l31;
  if (on >= a.N) return;
  const int ob = on / a.HW, op = on - ob * a.HW;
  float* yp = a.y + (long)ob * a.M * a.HW + op;
#pragma unroll
  for (int b = 0; b < MB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = m0 + 32 * b + 4 * h + (r & 3) + 8 * (r >> 2);
      if (o < a.M) yp[(long)o * a.HW] = acc[b][r] + (a.bias ? a.bias[o] : 0.f);
    }
}

struct C1WgradArgs {
  const float* x; const float* dy; float* part;
  int N, HW, Cin, Cout, klen;     // klen: pixels per split (a multiple of 32)
};

// A 64 (planes) x 32 (pixels k0 .. k0 + 31) tile of an NCHW tensor with C planes into 8 registers, and on to LDS as T[pixel][plane]
// (row stride 65, as gemm.hip's tiles)
__device__ __forceinline__ void c1_tile_load(const float* __restrict__ P, int C, int HW, int row0, int k0, int kend, bool vec, float (&v)[8], int tid) {
  if (vec) {
    const int n = k0 + (tid & 7) * 4;
    const bool in = n < kend;       // (kend % 4 == 0 on this path)
    const int b = in ? n / HW : 0, p = in ? n - b * HW : 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (tid >> 3) + 32 * i;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in && row0 + r < C) t = *reinterpret_cast<const float4*>(P + ((long)b * C + row0 + r) * HW + p);
      v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
  } else {
    const int n = k0 + (tid & 31);
    const bool in = n < kend;
    const int b = in ? n / HW : 0, p = in ? n - b * HW : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = (tid >> 5) + 8 * i;
      v[i] = (in && row0 + r < C) ? P[((long)b * C + row0 + r) * HW + p] : 0.f;
    }
  }
}
__device__ __forceinline__ void c1_tile_store(float* T, bool vec, const float (&v)[8], int tid) {
  if (vec) {
    const int k = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = (tid >> 3) + 32 * i;
#pragma unroll
      for (int j = 0; j < 4; ++j) T[(k + j) * 65 + r] = v[4 * i + j];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) T[(tid & 31) * 65 + (tid >> 5) + 8 * i] = v[i];
  }
}

__global__ __launch_bounds__(256) void conv1x1_wgrad_kernel(C1WgradArgs a) {
  __shared__ float As[32 * 65];
  __shared__ float Bs[32 * 65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int i0 = blockIdx.x * 64, o0 = blockIdx.y * 64;
  const int kbeg = blockIdx.z * a.klen, kend = min(a.N, kbeg + a.klen);
  const bool vec = (a.HW & 3) == 0 && (((uintptr_t)a.x | (uintptr_t)a.dy) & 15) == 0;
  c1_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float av[8], bv[8];
  c1_tile_load(a.dy, a.Cout, a.HW, o0, kbeg, kend, vec, av, tid);
  c1_tile_load(a.x, a.Cin, a.HW, i0, kbeg, kend, vec, bv, tid);
  for (int k0 = kbeg; k0 < kend; k0 += 32) {
    c1_tile_store(As, vec, av, tid);
    c1_tile_store(Bs, vec, bv, tid);
    __syncthreads();
    if (k0 + 32 < kend) {
      c1_tile_load(a.dy, a.Cout, a.HW, o0, k0 + 32, kend, vec, av, tid);
      c1_tile_load(a.x, a.Cin, a.HW, i0, k0 + 32, kend, vec, bv, tid);
    }
#pragma unroll
    for (int kk = 0; kk < 32; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + h) * 65 + wm * 32 + l31], Bs[(kk + h) * 65 + wn * 32 + l31], acc, 0, 0, 0);
    __syncthreads();
  }
  // every split writes every (o, i) of its tile that lies inside the matrix: the reduction reads all of them
  float* slab = a.part + (long)blockIdx.z * a.Cout * a.Cin;
  const int i = i0 + wn * 32 + l31;
  if (i >= a.Cin) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = o0 + wm * 32 + 4 * h + (r & 3) + 8 * (r >> 2);
    if (o < a.Cout) slab[(long)o * a.Cin + i] = acc[r];
  }
}

__global__ void conv1x1_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, long n, int splits) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  int k = 0;
  for (; k + 16 <= splits; k += 16) {      // sixteen loads in flight, then their sum in split order (one dependent load per add ran at one memory latency per slab)
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = part[(long)(k + j) * n + e];
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
  }
  for (; k < splits; ++k) s += part[(long)k * n + e];      // split order: deterministic
  gw[e] += s;
}

// Splits of the pixel axis: enough workgroups to fill the device (about 1024 with the channel tiles), at most 512, at least 32 pixels each
constexpr int C1_MAX_WGS = 1024, C1_MAX_SPLITS = 512;
static int c1_split_cap(int Cin, int Cout) {
  const long tiles = (long)((Cin + 63) / 64) * ((Cout + 63) / 64);
  const long cap = C1_MAX_WGS / tiles;
  return (int)(cap < 1 ? 1 : (cap > C1_MAX_SPLITS ? C1_MAX_SPLITS : cap));
}
size_t conv1x1_workspace_bytes(int B, int Cin, int Cout) { return sizeof(float) * (size_t)c1_split_cap(Cin, Cout) * Cin * Cout + 256; }

template <bool WK>
static void c1_launch(const C1Args& a, hipStream_t s) {
  const unsigned gx = (unsigned)((a.N + C1_NT - 1) / C1_NT);
  if (a.M <= 32) conv1x1_kernel<1, WK><<<dim3(gx, 1), 256, 0, s>>>(a);
  else if (a.M <= 64) conv1x1_kernel<2, WK><<<dim3(gx, 1), 256, 0, s>>>(a);
  else conv1x1_kernel<4, WK><<<dim3(gx, (unsigned)((a.M + 127) / 128)), 256, 0, s>>>(a);
}

// out[b,o,p] = bias[o] + sum_i w[o,i] in[b,i,p]
void launch_conv1x1_forward(const float* in, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW, hipStream_t s) {
  KtScope kt("conv1x1_kernel", 2.0 * B * HW * (double)Cin * Cout, 4.0 * B * HW * (Cin + Cout), s);
  c1_launch<true>(C1Args{in, w, bias, out, B * HW, HW, Cin, Cout, Cin, 1}, s);
}
// gin[b,i,p] = sum_o w[o,i] gout[b,o,p]
void launch_conv1x1_backward_data(const float* gout, const float* w, float* gin, int B, int Cin, int Cout, int HW, hipStream_t s) {
  KtScope kt("conv1x1_kernel(dgrad)", 2.0 * B * HW * (double)Cin * Cout, 4.0 * B * HW * (Cin + Cout), s);
  c1_launch<false>(C1Args{gout, w, nullptr, gin, B * HW, HW, Cout, Cin, 1, Cin}, s);
}
// gw[o,i] += sum_{b,p} gout[b,o,p] in[b,i,p]        (ws: conv1x1_workspace_bytes)
void launch_conv1x1_backward_weight(const float* in, const float* gout, float* gw, void* ws, int B, int Cin, int Cout, int HW, hipStream_t s) {
  const int N = B * HW, cap = c1_split_cap(Cin, Cout);
  int want = (N + 31) / 32; if (want > cap) want = cap;
  const int klen = round_up((N + want - 1) / want, 32), splits = (N + klen - 1) / klen;      // every split owns at least one pixel
  float* part = static_cast<float*>(ws);
  {
    KtScope kt("conv1x1_wgrad_kernel", 2.0 * N * (double)Cin * Cout, 4.0 * N * (Cin + Cout), s);
    conv1x1_wgrad_kernel<<<dim3((Cin + 63) / 64, (Cout + 63) / 64, splits), 256, 0, s>>>(C1WgradArgs{in, gout, part, N, HW, Cin, Cout, klen});
  }
  const long n = (long)Cin * Cout;
  KtScope kt("conv1x1_wgrad_reduce_kernel", (double)n * splits, 4.0 * n * (splits + 2), s);
  conv1x1_wgrad_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(part, gw, n, splits);
}

}  // namespace gr
