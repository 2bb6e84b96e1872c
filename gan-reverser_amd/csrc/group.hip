// group.hip — the grouped layer kinds that let models.create_G4 (reference models.lua:145-194) run as ONE gr_net: its nn.Concat(2) of 32
// structurally identical branches is a chain of grouped operators over the concatenated features.
//   GR_GROUPLINEAR  G block-diagonal nn.Linear: group g reads inputs [g a/G, (g+1) a/G) and writes outputs [g b/G, (g+1) b/G);
//                   weight [b][a/G] (the branches' matrices one after another), bias [b]
//   GR_GROUPCONV3   3x3 stride-1 pad-1 convolution with G groups, weight [b][a/G][3][3] (cudnn.SpatialConvolution's `groups` layout); behind
//                   an nn.SpatialUpSamplingNearest(2) the kernels index the half-size input themselves (in[y >> 1][x >> 1]; the data
//                   gradient sums its 2x2 block): no up-sampled tensor exists
//   GR_PRELU, n >= 2 slopes: slope j covers channels [j C/n, (j+1) C/n)
// All of it is fp32 on the vector ALU with fp32 accumulation - what this file launches is exact fp32 in every GR_CONV_MODE, like convk.hip
// and conv1x1.hip.  That no longer holds for the GR_GROUPCONV3 stage as a whole: with 16 planes per group on both sides and planes up to
// 32 x 32 (G4's instance), from group_mfma_min_tiles (image, group) tiles on and outside f32 mode, net.hip takes groupmfma.hip's f16x3 /
// bf16x6 MFMA launches instead; every other shape, small batches and f32 mode run here.
// Every reduction runs in a fixed order (per thread, then a fixed tree, then partials in index order by a second launch): no float atomics,
// two runs give the same bits.  The bias gradients are not computed here: like every stage's, they come from the pipeline backward.
#include "kernels.h"

namespace gr {

// ---------------------------------------------------------------------------------------------------------------- grouped Linear
constexpr int GL_BT = 8;          // batch rows per thread (forward) : the weight row is read once per GL_BT rows
constexpr int GL_KC = 16;         // inputs per register chunk (data / weight gradient)

// y[bi][o] = bias[o] + sum_k W[o][k] x[bi][g Kg + k],  g = o / Mg.  One thread per output column, GL_BT batch rows each.
__global__ __launch_bounds__(256) void grouplinear_forward_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                  float* __restrict__ y, int B, int a, int b, int Kg, int Mg) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= b) return;
  const int b0 = blockIdx.y * GL_BT;
  const float* xg = x + (long)(o / Mg) * Kg;
  const float* wr = w + (long)o * Kg;
  float acc[GL_BT];
  const float bv = bias[o];
#pragma unroll
  for (int r = 0; r < GL_BT; ++r) acc[r] = bv;
  for (int k = 0; k < Kg; ++k) {
    const float wv = wr[k];
#pragma unroll
    for (int r = 0; r < GL_BT; ++r)
      if (b0 + r < B) acc[r] = fmaf(wv, xg[(long)(b0 + r) * a + k], acc[r]);
  }
#pragma unroll
  for (int r = 0; r < GL_BT; ++r)
    if (b0 + r < B) y[(long)(b0 + r) * b + o] = acc[r];
}

// sum of v over the 256 threads of the workgroup in a fixed order (wave butterflies, then the four waves in index order); valid in thread 0
__device__ __forceinline__ float block_sum_256(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                                  // (sh may still be read by the previous call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

constexpr int GL_DB = 4;          // batch rows per workgroup (data gradient): the weight rows are read once per GL_DB rows
// gin[bi][g Kg + k] = sum_{o in group g} gout[bi][o] W[o][k].  Workgroup = (group g, GL_DB batch rows); its threads stride over the group's Mg outputs.
__global__ __launch_bounds__(256) void grouplinear_dgrad_kernel(const float* __restrict__ gout, const float* __restrict__ w, float* __restrict__ gin,
                                                                int B, int a, int b, int Kg, int Mg) {
  __shared__ float sh[4];
  const int g = blockIdx.x, b0 = blockIdx.y * GL_DB;
  for (int k0 = 0; k0 < Kg; k0 += GL_KC) {
    float acc[GL_DB][GL_KC];
#pragma unroll
    for (int r = 0; r < GL_DB; ++r)
#pragma unroll
      for (int k = 0; k < GL_KC; ++k) acc[r][k] = 0.f;
    for (int m = threadIdx.x; m < Mg; m += 256) {
      const long o = (long)g * Mg + m;
      float gv[GL_DB];
#pragma unroll
      for (int r = 0; r < GL_DB; ++r) gv[r] = b0 + r < B ? gout[(long)(b0 + r) * b + o] : 0.f;
#pragma unroll
      for (int k = 0; k < GL_KC; ++k) {
        const float wv = k0 + k < Kg ? w[o * Kg + k0 + k] : 0.f;
#pragma unroll
        for (int r = 0; r < GL_DB; ++r) acc[r][k] = fmaf(gv[r], wv, acc[r][k]);
      }
    }
#pragma unroll
    for (int r = 0; r < GL_DB; ++r)
#pragma unroll
      for (int k = 0; k < GL_KC; ++k) {
        const float s = block_sum_256(acc[r][k], sh);
        if (threadIdx.x == 0 && b0 + r < B && k0 + k < Kg) gin[(long)(b0 + r) * a + (long)g * Kg + k0 + k] = s;
      }
  }
}

// gW[o][k] += sum_bi gout[bi][o] x[bi][g Kg + k]: one thread per output row o, the batch in order
__global__ __launch_bounds__(256) void grouplinear_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gout, float* __restrict__ gw,
                                                                int B, int a, int b, int Kg, int Mg) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= b) return;
  const float* xg = x + (long)(o / Mg) * Kg;
  for (int k0 = 0; k0 < Kg; k0 += GL_KC) {
    float acc[GL_KC];
#pragma unroll
    for (int k = 0; k < GL_KC; ++k) acc[k] = 0.f;
    for (int bi = 0; bi < B; ++bi) {
      const float gv = gout[(long)bi * b + o];
#pragma unroll
      for (int k = 0; k < GL_KC; ++k)
        if (k0 + k < Kg) acc[k] = fmaf(gv, xg[(long)bi * a + k0 + k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < GL_KC; ++k)
      if (k0 + k < Kg) gw[(long)o * Kg + k0 + k] += acc[k];
  }
}

void launch_grouplinear_forward(const float* x, const float* w, const float* bias, float* y, int B, int a, int b, int G, hipStream_t s) {
  KtScope kt("grouplinear_forward_kernel", 2.0 * B * (double)b * (a / G), 4.0 * ((double)B * (a + b) + (double)b * (a / G)), s);
  grouplinear_forward_kernel<<<dim3((unsigned)((b + 255) / 256), (unsigned)((B + GL_BT - 1) / GL_BT)), 256, 0, s>>>(x, w, bias, y, B, a, b, a / G, b / G);
}
void launch_grouplinear_backward_data(const float* gout, const float* w, float* gin, int B, int a, int b, int G, hipStream_t s) {
  KtScope kt("grouplinear_dgrad_kernel", 2.0 * B * (double)b * (a / G), 4.0 * ((double)B * (a + b) + (double)b * (a / G)), s);
  grouplinear_dgrad_kernel<<<dim3((unsigned)G, (unsigned)((B + GL_DB - 1) / GL_DB)), 256, 0, s>>>(gout, w, gin, B, a, b, a / G, b / G);
}
void launch_grouplinear_backward_weight(const float* x, const float* gout, float* gw, int B, int a, int b, int G, hipStream_t s) {
  KtScope kt("grouplinear_wgrad_kernel", 2.0 * B * (double)b * (a / G), 4.0 * ((double)B * (a + b) + 2.0 * b * (a / G)), s);
  grouplinear_wgrad_kernel<<<(unsigned)((b + 255) / 256), 256, 0, s>>>(x, gout, gw, B, a, b, a / G, b / G);
}

// ---------------------------------------------------------------------------------------------------------------- grouped 3x3 convolution
constexpr int GC_OC = 16;         // output planes per register chunk (forward)
constexpr int GC_CI = 8;          // input planes per register chunk (data gradient)
constexpr int GC_WO = 8;          // output planes per workgroup (weight gradient)

struct GcArgs {
  const float* in; const float* w; const float* bias; float* out;
  int B, Cin, Cout, Cg, Og, H, W, up;        // H x W: the convolution's planes; up: `in` is [B][Cin][H/2][W/2]
};
// The nine taps of the pixel (y, x) of the convolution's H x W plane as offsets into the stored input plane (in[yy >> 1][xx >> 1] behind an
// up-sampling) and 0 / 1 marks for the zero padding: computed once per pixel, used for every plane and image (an offset of a padded tap is 0)
__device__ __forceinline__ void gc_taps(int y, int x, int H, int W, int up, int (&off)[9], float (&m)[9]) {
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
    off[t] = !in ? 0 : up ? (yy >> 1) * (W >> 1) + (xx >> 1) : yy * W + xx;
    m[t] = in ? 1.f : 0.f;
  }
}

// out[bi][g Og + oc][y][x] = bias + sum_{ci < Cg, ky, kx} W[g Og + oc][ci][ky][kx] in[bi][g Cg + ci][y + ky - 1][x + kx - 1]
// grid (pixel tiles, G, B); one thread per pixel, GC_OC output planes at a time (the weights are uniform over the workgroup)
__global__ __launch_bounds__(256) void groupconv3_forward_kernel(GcArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, bi = blockIdx.z;
  if (p >= a.H * a.W) return;
  const int y = p / a.W, x = p - y * a.W;
  int off[9]; float m[9];
  gc_taps(y, x, a.H, a.W, a.up, off, m);
  const long in_hw = a.up ? (long)(a.H >> 1) * (a.W >> 1) : (long)a.H * a.W;
  const float* inb = a.in + ((long)bi * a.Cin + (long)g * a.Cg) * in_hw;
  for (int oc0 = 0; oc0 < a.Og; oc0 += GC_OC) {
    float acc[GC_OC];
#pragma unroll
    for (int j = 0; j < GC_OC; ++j) acc[j] = oc0 + j < a.Og ? a.bias[g * a.Og + oc0 + j] : 0.f;
    for (int ci = 0; ci < a.Cg; ++ci) {
      const float* plane = inb + ci * in_hw;
      float v[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) v[t] = m[t] != 0.f ? plane[off[t]] : 0.f;
#pragma unroll
      for (int j = 0; j < GC_OC; ++j) {
        if (oc0 + j < a.Og) {
          const float* wp = a.w + ((long)(g * a.Og + oc0 + j) * a.Cg + ci) * 9;
#pragma unroll
          for (int t = 0; t < 9; ++t) acc[j] = fmaf(wp[t], v[t], acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GC_OC; ++j)
      if (oc0 + j < a.Og) a.out[((long)bi * a.Cout + g * a.Og + oc0 + j) * a.H * a.W + p] = acc[j];
  }
}

// gin[bi][g Cg + ci][yi][xi] = sum over the 1 (or, behind an up-sampling, 2x2) convolution-plane pixels (y, x) this input pixel feeds of
//   sum_{oc < Og, ky, kx} gout[bi][g Og + oc][y - ky + 1][x - kx + 1] W[g Og + oc][ci][ky][kx]
// a.in = gout, a.out = gin; grid (input-pixel tiles, G, B); one thread per input pixel, GC_CI input planes at a time.  The gradOutput
// neighbourhood of the pixel - 3 x 3, or the 4 x 4 block around its 2 x 2 - is loaded once per output plane (offsets and padding factors
// once per pixel) and serves every tap of every sub-pixel: sub-pixel (sy, sx), tap (ky, kx) reads neighbourhood entry (sy - ky + 2, sx - kx + 2).
template <int UP>
__global__ __launch_bounds__(256) void groupconv3_dgrad_kernel(GcArgs a) {
  constexpr int NS = UP ? 2 : 1, NB = UP ? 4 : 3;        // sub-pixels per side, neighbourhood side
  const int Hi = UP ? a.H >> 1 : a.H, Wi = UP ? a.W >> 1 : a.W;
  const int p = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, bi = blockIdx.z;
  if (p >= Hi * Wi) return;
  const int yi = p / Wi, xi = p - yi * Wi;
  int off[NB * NB]; float m[NB * NB];
#pragma unroll
  for (int e = 0; e < NB * NB; ++e) {
    const int yy = (UP ? 2 * yi : yi) + e / NB - 1, xx = (UP ? 2 * xi : xi) + e % NB - 1;
    const bool in = yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
    off[e] = in ? yy * a.W + xx : 0;
    m[e] = in ? 1.f : 0.f;
  }
  const long hw = (long)a.H * a.W;
  const float* gb = a.in + ((long)bi * a.Cout + (long)g * a.Og) * hw;
  for (int ci0 = 0; ci0 < a.Cg; ci0 += GC_CI) {
    float acc[GC_CI];
#pragma unroll
    for (int j = 0; j < GC_CI; ++j) acc[j] = 0.f;
    for (int oc = 0; oc < a.Og; ++oc) {
      const float* plane = gb + oc * hw;
      float v[NB * NB];
#pragma unroll
      for (int e = 0; e < NB * NB; ++e) v[e] = m[e] != 0.f ? plane[off[e]] : 0.f;
#pragma unroll
      for (int j = 0; j < GC_CI; ++j) {
        if (ci0 + j < a.Cg) {
          const float* wp = a.w + ((long)(g * a.Og + oc) * a.Cg + ci0 + j) * 9;
#pragma unroll
          for (int sy = 0; sy < NS; ++sy)
#pragma unroll
            for (int sx = 0; sx < NS; ++sx)
#pragma unroll
              for (int t = 0; t < 9; ++t) acc[j] = fmaf(wp[t], v[(sy - t / 3 + 2) * NB + (sx - t % 3 + 2)], acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GC_CI; ++j)
      if (ci0 + j < a.Cg) a.out[((long)bi * a.Cin + g * a.Cg + ci0 + j) * Hi * Wi + p] = acc[j];
  }
}

// part[split][o][ci][t] = sum over the split's images and every pixel of gout[bi][o][y][x] in[bi][g Cg + ci][y + ky - 1][x + kx - 1]
// grid (Cin = (g, ci), chunks of GC_WO output planes of the group, splits).  A thread owns pixels (their tap offsets computed once) and walks
// the split's images: 9 input values and GC_WO gradOutput values per (pixel, image) feed 9 x GC_WO accumulators.
__global__ __launch_bounds__(256) void groupconv3_wgrad_kernel(GcArgs a, const float* __restrict__ gout, float* __restrict__ part, int per_split) {
  __shared__ float sh[4];
  const int g = blockIdx.x / a.Cg, ci = blockIdx.x - g * a.Cg, oc0 = blockIdx.y * GC_WO, split = blockIdx.z;
  const int bbeg = split * per_split, bend = min(a.B, bbeg + per_split);
  const int hw = a.H * a.W;
  const long in_hw = a.up ? (long)(a.H >> 1) * (a.W >> 1) : (long)hw;
  float acc[GC_WO][9];
#pragma unroll
  for (int j = 0; j < GC_WO; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = 0.f;
  for (int p = threadIdx.x; p < hw; p += 256) {
    const int y = p / a.W, x = p - y * a.W;
    int off[9]; float m[9];
    gc_taps(y, x, a.H, a.W, a.up, off, m);
    for (int bi = bbeg; bi < bend; ++bi) {
      const float* plane = a.in + ((long)bi * a.Cin + blockIdx.x) * in_hw;
      const float* gp = gout + ((long)bi * a.Cout + (long)g * a.Og + oc0) * hw + p;
      float v[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) v[t] = m[t] != 0.f ? plane[off[t]] : 0.f;
#pragma unroll
      for (int j = 0; j < GC_WO; ++j) {
        if (oc0 + j < a.Og) {
          const float gv = gp[(long)j * hw];
#pragma unroll
          for (int t = 0; t < 9; ++t) acc[j][t] = fmaf(gv, v[t], acc[j][t]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < GC_WO; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float s = block_sum_256(acc[j][t], sh);
      if (threadIdx.x == 0 && oc0 + j < a.Og) part[(((long)split * a.Cout + g * a.Og + oc0 + j) * a.Cg + ci) * 9 + t] = s;
    }
}
// gw[e] += the splits' partials in split order
__global__ void group_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, long n, int splits) {
  const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[(long)k * n + e];
  gw[e] += s;
}

constexpr int GC_MAX_SPLITS = 16;
static int gc_splits(int B) { return B < GC_MAX_SPLITS ? B : GC_MAX_SPLITS; }
size_t groupconv3_workspace_bytes(int B, int Cin, int Cout, int G) { return sizeof(float) * (size_t)gc_splits(B) * Cout * (Cin / G) * 9 + 256; }

static GcArgs gc_args(const float* in, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int G, int H, int W, bool up) {
  return GcArgs{in, w, bias, out, B, Cin, Cout, Cin / G, Cout / G, H, W, up ? 1 : 0};
}
static double gc_flops(int B, int Cin, int Cout, int G, int H, int W) { return 2.0 * B * H * W * (double)Cout * (Cin / G) * 9; }
static double gc_bytes(int B, int Cin, int Cout, int H, int W, bool up) { return 4.0 * B * ((double)Cin * H * W / (up ? 4 : 1) + (double)Cout * H * W); }

void launch_groupconv3_forward(const float* in, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int G, int H, int W, bool up, hipStream_t s) {
  KtScope kt("groupconv3_forward_kernel", gc_flops(B, Cin, Cout, G, H, W), gc_bytes(B, Cin, Cout, H, W, up), s);
  groupconv3_forward_kernel<<<dim3((unsigned)((H * W + 255) / 256), (unsigned)G, (unsigned)B), 256, 0, s>>>(gc_args(in, w, bias, out, B, Cin, Cout, G, H, W, up));
}
void launch_groupconv3_backward_data(const float* gout, const float* w, float* gin, int B, int Cin, int Cout, int G, int H, int W, bool up, hipStream_t s) {
  KtScope kt("groupconv3_dgrad_kernel", gc_flops(B, Cin, Cout, G, H, W), gc_bytes(B, Cin, Cout, H, W, up), s);
  const int hwi = up ? (H / 2) * (W / 2) : H * W;
  const dim3 grid((unsigned)((hwi + 255) / 256), (unsigned)G, (unsigned)B);
  if (up) groupconv3_dgrad_kernel<1><<<grid, 256, 0, s>>>(gc_args(gout, w, nullptr, gin, B, Cin, Cout, G, H, W, up));
  else groupconv3_dgrad_kernel<0><<<grid, 256, 0, s>>>(gc_args(gout, w, nullptr, gin, B, Cin, Cout, G, H, W, up));
}
void launch_groupconv3_backward_weight(const float* in, const float* gout, float* gw, void* ws, int B, int Cin, int Cout, int G, int H, int W, bool up, hipStream_t s) {
  const int splits = gc_splits(B), per = (B + splits - 1) / splits, used = (B + per - 1) / per;      // every split owns at least one image
  float* part = static_cast<float*>(ws);
  {
    KtScope kt("groupconv3_wgrad_kernel", gc_flops(B, Cin, Cout, G, H, W), gc_bytes(B, Cin, Cout, H, W, up), s);
    groupconv3_wgrad_kernel<<<dim3((unsigned)Cin, (unsigned)((Cout / G + GC_WO - 1) / GC_WO), (unsigned)used), 256, 0, s>>>(
        gc_args(in, nullptr, nullptr, nullptr, B, Cin, Cout, G, H, W, up), gout, part, per);
  }
  const long n = (long)Cout * (Cin / G) * 9;
  KtScope kt("group_wgrad_reduce_kernel", (double)n * used, 4.0 * n * (used + 2), s);
  group_wgrad_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(part, gw, n, used);
}

// ---------------------------------------------------------------------------------------------------------------- nn.PReLU with n >= 2 slopes
// x [B][C][HW]; slope j covers channels [j C/n, (j+1) C/n): L = (C/n) HW consecutive elements of every sample.  y = x > 0 ? x : w_j x (THNN PReLU.c)
__global__ __launch_bounds__(256) void prelu_multi_forward_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, long n, long L, int ns) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += 256L * gridDim.x) {
    const float v = x[e];
    y[e] = v > 0.f ? v : w[(e / L) % ns] * v;
  }
}
// gin = x > 0 ? g : w_j g
__global__ __launch_bounds__(256) void prelu_multi_backward_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ w,
                                                                   float* __restrict__ gin, long n, long L, int ns) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += 256L * gridDim.x) gin[e] = x[e] > 0.f ? g[e] : w[(e / L) % ns] * g[e];
}
// gw[j] += sum over slope j's elements with x <= 0 of g x: products in fp32, sums in fp64 - per thread, per workgroup, then the workgroups'
// partials of a slope in index order by the second launch (launch_prelu_grad's rule).  grid (parts, ns)
constexpr int PM_PARTS = 64;
__global__ __launch_bounds__(256) void prelu_multi_grad_partial_kernel(const float* __restrict__ g, const float* __restrict__ x, int B, long L, int ns, double* __restrict__ part) {
  __shared__ double sh[256];
  const int j = blockIdx.y;
  const long total = (long)B * L;
  double s = 0;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += 256L * gridDim.x) {
    const long bi = e / L, at = (bi * ns + j) * L + (e - bi * L);
    const float xv = x[at];
    if (!(xv > 0.f)) s += (double)(g[at] * xv);
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) { if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w]; __syncthreads(); }
  if (threadIdx.x == 0) part[(long)j * gridDim.x + blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(64) void prelu_multi_grad_final_kernel(const double* __restrict__ part, int nparts, int ns, float* __restrict__ gw) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= ns) return;
  double s = 0;
  for (int k = 0; k < nparts; ++k) s += part[(long)j * nparts + k];
  gw[j] += (float)s;
}
static unsigned pm_blocks(long n) { long b = (n + 1023) / 1024; return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }
void launch_prelu_multi_forward(const float* x, const float* w, float* y, int B, int C, int HW, int ns, hipStream_t s) {
  const long n = (long)B * C * HW;
  KtScope kt("prelu_multi_forward_kernel", (double)n, 8.0 * n, s);
  prelu_multi_forward_kernel<<<pm_blocks(n), 256, 0, s>>>(x, w, y, n, (long)(C / ns) * HW, ns);
}
void launch_prelu_multi_backward(const float* g, const float* x, const float* w, float* gin, int B, int C, int HW, int ns, hipStream_t s) {
  const long n = (long)B * C * HW;
  KtScope kt("prelu_multi_backward_kernel", (double)n, 12.0 * n, s);
  prelu_multi_backward_kernel<<<pm_blocks(n), 256, 0, s>>>(g, x, w, gin, n, (long)(C / ns) * HW, ns);
}
size_t prelu_multi_grad_workspace_bytes(int ns) { return sizeof(double) * (size_t)ns * PM_PARTS; }
void launch_prelu_multi_grad(const float* g, const float* x, int B, int C, int HW, int ns, double* part, float* gw, hipStream_t s) {
  const long L = (long)(C / ns) * HW, total = (long)B * L;
  long parts = (total + 1023) / 1024;
  if (parts < 1) parts = 1;
  if (parts > PM_PARTS) parts = PM_PARTS;
  KtScope kt("prelu_multi_grad_kernel", 2.0 * B * C * HW, 8.0 * B * C * HW, s);
  prelu_multi_grad_partial_kernel<<<dim3((unsigned)parts, (unsigned)ns), 256, 0, s>>>(g, x, B, L, ns, part);
  prelu_multi_grad_final_kernel<<<(unsigned)((ns + 63) / 64), 64, 0, s>>>(part, (int)parts, ns, gw);
}

}  // namespace gr
