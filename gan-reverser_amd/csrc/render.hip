// render.hip — the pictures apply_r.lua and sample.lua end in, rendered where the images lie.
// Compiled with -ffp-contract=off: every value below is produced by single IEEE fp32 operations in the order include/ganrev.h states
// (gr_image_grid_dev, gr_rows_mean_dev), so tests/imagegrid_oracle.py matches these kernels bit for bit.
//
// Replaces (reference file:line):
//   image.toDisplayTensor{input, nrow, min, max}            apply_r.lua:137,256,297,341,346,350,388; sample.lua:167,184
//   NN_UTILS.toRgb / toRgbSingle before it                  apply_r.lua:255,284,334-335,385; sample.lua:167,184
//   the blue frame drawn over the needle                    apply_r.lua:286-295
//   the blue field of the pairs, the red / black frames     apply_r.lua:325-326,375-383
//   face:add(img) ... face:div(n)                           apply_r.lua:233-243
//
// These kernels move a few megabytes at most: one thread per output pixel, full output rows written by consecutive lanes, the per-tile
// metadata read from a small device array (every lane of a tile row reads the same 32 bytes).  Nothing here is tuned beyond that.
#include "kernels.h"
#include "colorspace.h"

namespace gr {

// NN_UTILS.toRgb of one pixel; `from` is uniform over a launch; -1 and CS_RGB copy the channels
__device__ __forceinline__ Px3 to_rgb_from(int from, Px3 x) {
  switch (from) {
    case CS_Y: return cs_to_rgb<CS_Y>(x);
    case CS_YUV: return cs_to_rgb<CS_YUV>(x);
    case CS_HSL: return cs_to_rgb<CS_HSL>(x);
    default: return x;
  }
}

// Output pixel (gy, gx) before the display range is applied: false = no tile covers it (it takes `fill`); true = v holds the tile's
// background (margin, or a slot whose row is -1) or the slot image's pixel, converted to rgb and with the inset frame drawn over it.
__device__ __forceinline__ bool grid_pixel(const GridGeom& g, int gy, int gx, Px3& v) {
  const int cy = gy / g.cellH, cx = gx / g.cellW;
  const int ty = gy - cy * g.cellH - g.padding / 2, tx = gx - cx * g.cellW - g.padding / 2;
  const int t = cy * g.xmaps + cx;
  if (ty < 0 || ty >= g.TH || tx < 0 || tx >= g.TW || t >= g.n_tiles) return false;
  const GridTile tl = g.tiles[t];
  v = Px3{tl.bg[0], tl.bg[1], tl.bg[2]};
  const int iy = ty - g.margin, ix = tx - g.margin;
  if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.slots * g.W) return true;
  const int s = ix >= g.W ? 1 : 0, px = ix - s * g.W;
  const long row = tl.row[s];
  if (row < 0) return true;
  const long hw = (long)g.H * g.W;
  const float* p = g.src[s] + row * g.C * hw + (long)iy * g.W + px;
  Px3 x{p[0], 0.f, 0.f};
  if (g.C == 3) { x.b = p[hw]; x.c = p[2 * hw]; }
  x = to_rgb_from(g.from, x);
  if (tl.inset && (iy == 0 || iy == g.H - 1 || px == 0 || px == g.W - 1)) x = Px3{g.inset_rgb[0], g.inset_rgb[1], g.inset_rgb[2]};
  v = x;
  return true;
}

// (min, max) over the workgroup by compare-selects (a NaN never wins); every thread receives the result.  sh: 8 floats.
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
    mn = a < mn ? a : mn; mx = b > mx ? b : mx;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[wave] = mn; sh[4 + wave] = mx; }
  __syncthreads();
  mn = sh[0]; mx = sh[4];
#pragma unroll
  for (int w = 1; w < 4; ++w) { mn = sh[w] < mn ? sh[w] : mn; mx = sh[4 + w] > mx ? sh[4 + w] : mx; }
}

// auto range, first launch: workgroup b leaves the (min, max) of its share of the pixels inside tiles in parts[2b], parts[2b + 1]
// (+inf / -inf for a share without any).  min and max do not depend on the order they are taken in; the sign of a zero does, and
// the grid kernel removes it.
__global__ __launch_bounds__(256) void image_grid_range_kernel(GridGeom g, float* __restrict__ parts) {
  __shared__ float sh[8];
  float mn = __builtin_inff(), mx = -__builtin_inff();
  const long npix = (long)g.GH * g.GW;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    const int gy = (int)(p / g.GW), gx = (int)(p - (long)gy * g.GW);
    Px3 v;
    if (!grid_pixel(g, gy, gx, v)) continue;
    mn = v.a < mn ? v.a : mn; mx = v.a > mx ? v.a : mx;
    if (g.Cout == 3) {
      mn = v.b < mn ? v.b : mn; mx = v.b > mx ? v.b : mx;
      mn = v.c < mn ? v.c : mn; mx = v.c > mx ? v.c : mx;
    }
  }
  block_minmax(mn, mx, sh);
  if (threadIdx.x == 0) { parts[2 * blockIdx.x] = mn; parts[2 * blockIdx.x + 1] = mx; }
}

// display value of a pixel inside a tile: clamp to [lo, hi], then (v - lo) / (hi - lo); 0 when hi == lo
__device__ __forceinline__ float grid_display(float v, float lo, float hi, float range) {
  float c = v < lo ? lo : v;
  c = c > hi ? hi : c;
  return range == 0.f ? 0.f : (c - lo) / range;
}
__device__ __forceinline__ uint8_t grid_quantise(float v) {
  float q = v * 255.f + 0.5f;                          // two operations: this file is not contracted
  q = q > 255.f ? 255.f : q;
  q = q > 0.f ? q : 0.f;                               // a negative or NaN fill
  return (uint8_t)(int)q;
}
// one thread per output pixel, all channels: grid [Cout][GH][GW] floats and / or u8 [GH][GW][Cout] bytes
__global__ __launch_bounds__(256) void image_grid_kernel(GridGeom g, const float* __restrict__ parts, int nparts,
                                                         float* __restrict__ grid, uint8_t* __restrict__ u8) {
  __shared__ float sh[8];
  float lo = g.lo, hi = g.hi;
  if (parts) {                                         // uniform: every thread of every workgroup reduces the same partial pairs
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
      const float a = parts[2 * i], b = parts[2 * i + 1];
      mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    block_minmax(mn, mx, sh);
    lo = mn + 0.f; hi = mx + 0.f;                      // -0 + 0 = +0: which zero a compare-select kept depends on the order, the sum does not
  }
  const long npix = (long)g.GH * g.GW;
  const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const int gy = (int)(p / g.GW), gx = (int)(p - (long)gy * g.GW);
  const float range = hi - lo;
  Px3 v;
  float o[3] = {g.fill, g.fill, g.fill};
  if (grid_pixel(g, gy, gx, v)) {
    o[0] = grid_display(v.a, lo, hi, range);
    if (g.Cout == 3) { o[1] = grid_display(v.b, lo, hi, range); o[2] = grid_display(v.c, lo, hi, range); }
  }
  for (int c = 0; c < g.Cout; ++c) {
    if (grid) grid[c * npix + p] = o[c];
    if (u8) u8[p * g.Cout + c] = grid_quantise(o[c]);
  }
}

void launch_image_grid(const GridGeom& g, float* parts, float* grid, uint8_t* u8, hipStream_t s) {
  const long npix = (long)g.GH * g.GW;
  const double tile_px = (double)g.n_tiles * g.TH * g.TW;
  int nparts = 0;
  if (parts) {
    long b = (npix + 255) / 256;
    nparts = (int)(b > GRID_RANGE_BLOCKS ? GRID_RANGE_BLOCKS : b);
    KtScope kt("image_grid_range_kernel", 0.0, 4.0 * g.C * tile_px, s);
    hipLaunchKernelGGL(image_grid_range_kernel, dim3((unsigned)nparts), dim3(256), 0, s, g, parts);
  }
  KtScope kt("image_grid_kernel", 0.0, 4.0 * g.C * tile_px + (double)npix * g.Cout * ((grid ? 4.0 : 0.0) + (u8 ? 1.0 : 0.0)), s);
  hipLaunchKernelGGL(image_grid_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, g, (const float*)parts, nparts, grid, u8);
}

// ------------------------------------------------------------------ the trainers' progress pictures (utils/nn_utils.lua:490-548)
// The ten digits as 3 x 5 blocks, one octal digit per pixel row from the top, the left pixel the high bit: the seven-segment shapes of
// utils/nn_utils.lua:430-479 ("1" is the right-hand column only, the middle bar of "3" starts in the middle column).
__constant__ const unsigned short PROGRESS_GLYPH[10] = {075557, 011111, 071747, 071317, 055711, 074717, 074757, 071111, 075757, 075717};

// pixel (gy, gx) of the seven bottom rows: true with v = 0 / 1 when a digit's block covers it (digit p = 1, 2, ... from the right covers
// columns GW-2-6p .. GW-6p of rows GH-7 .. GH-3)
__device__ __forceinline__ bool progress_digit(const ProgressGeom& g, int gy, int gx, float& v) {
  const int r = gy - (g.GH - 7), d = g.GW - gx;          // d = 6p + 2 at the block's left column, 6p at its right
  const int p = d / 6, k = d - 6 * p;
  if (r < 0 || r > 4 || p < 1 || p > g.ndig || k > 2) return false;
  v = (float)((PROGRESS_GLYPH[g.dig[p - 1]] >> (3 * (4 - r) + k)) & 1);
  return true;
}
// the N (1 or 4) pixels (gy, gx ..) of one cell row: cell (gy / H, gx / W); N = 4 asks W % 4 == 0, so that they share the cell
template <int N>
__device__ __forceinline__ void progress_pixels(const ProgressGeom& g, int gy, int gx, float (&o)[3][N]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < N; ++j) o[c][j] = 0.f;
  if (gy >= g.GH - 7) {                                  // the bottom rows: zeros and the digits
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float v;
      if (progress_digit(g, gy, gx + j, v)) o[0][j] = o[1][j] = o[2][j] = v;
    }
    return;
  }
  const int cy = gy / g.H, cx = gx / g.W, t = cy * g.grid_w + cx;
  if (t >= g.n_cells) return;
  const long hw = (long)g.H * g.W;
  const float* p = g.src + g.rows[t] * g.C * hw + (long)(gy - cy * g.H) * g.W + (gx - cx * g.W);
  float x[3][N];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (c < g.C) {
      if constexpr (N == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + c * hw);
        x[c][0] = q.x; x[c][1] = q.y; x[c][2] = q.z; x[c][3] = q.w;
      } else {
        x[c][0] = p[c * hw];
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) x[c][j] = 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const Px3 v = to_rgb_from(g.from, Px3{x[0][j], x[1][j], x[2][j]});
    o[0][j] = v.a; o[1][j] = v.b; o[2][j] = v.c;
  }
}
// one thread per N pixels of a grid row, all channels: grid [Cout][GH][GW] floats (the values as they are) and / or u8 [GH][GW][Cout]
// bytes (display range [0, 1]).  N = 4: one 16-byte store per channel of the grid, the 4 Cout bytes of u8 as Cout words.
template <int N>
__global__ __launch_bounds__(256) void progress_grid_kernel(ProgressGeom g, float* __restrict__ grid, uint8_t* __restrict__ u8) {
  const long npix = (long)g.GH * g.GW;
  const long p = (blockIdx.x * (long)blockDim.x + threadIdx.x) * N;
  if (p >= npix) return;
  const int gy = (int)(p / g.GW), gx = (int)(p - (long)gy * g.GW);
  float o[3][N];
  progress_pixels<N>(g, gy, gx, o);
  if (grid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= g.Cout) break;
      if constexpr (N == 4) *reinterpret_cast<float4*>(grid + c * npix + p) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
      else grid[c * npix + p] = o[c][0];
    }
  }
  if (u8) {
    uint32_t q[3][N];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < N; ++j) q[c][j] = grid_quantise(grid_display(o[c][j], 0.f, 1.f, 1.f));
    uint8_t* d = u8 + p * g.Cout;
    if constexpr (N == 4) {                              // the 4 Cout bytes as they lie in u8: pixel-major, channel-minor
      uint32_t* w = reinterpret_cast<uint32_t*>(d);
      if (g.Cout == 1) {
        w[0] = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[0][3] << 24);
      } else {
        w[0] = q[0][0] | (q[1][0] << 8) | (q[2][0] << 16) | (q[0][1] << 24);
        w[1] = q[1][1] | (q[2][1] << 8) | (q[0][2] << 16) | (q[1][2] << 24);
        w[2] = q[2][2] | (q[0][3] << 8) | (q[1][3] << 16) | (q[2][3] << 24);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c < g.Cout) d[c] = (uint8_t)q[c][0];
    }
  }
}
void launch_progress_grid(const ProgressGeom& g, bool vec, float* grid, uint8_t* u8, hipStream_t s) {
  const long npix = (long)g.GH * g.GW, threads = vec ? npix / 4 : npix;
  KtScope kt("progress_grid_kernel", 0.0, 4.0 * g.C * (double)g.n_cells * g.H * g.W + (double)npix * g.Cout * ((grid ? 4.0 : 0.0) + (u8 ? 1.0 : 0.0)), s);
  const dim3 blocks((unsigned)((threads + 255) / 256));
  if (vec) hipLaunchKernelGGL(progress_grid_kernel<4>, blocks, dim3(256), 0, s, g, grid, u8);
  else hipLaunchKernelGGL(progress_grid_kernel<1>, blocks, dim3(256), 0, s, g, grid, u8);
}

// ------------------------------------------------------------------ a cluster's average face (apply_r.lua:233-243)
// torch.zeros(...), face:add(img) once per image in list order, face:div(n): a sequential fp32 sum and ONE division, per pixel.
__global__ __launch_bounds__(256) void rows_mean_kernel(const float* __restrict__ x, long d, const long* __restrict__ rows, int n, float* __restrict__ out) {
  const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (p >= d) return;
  float acc = 0.f;
  for (int j = 0; j < n; ++j) acc = acc + x[rows[j] * d + p];
  out[p] = n > 0 ? acc / (float)n : 0.f;
}
void launch_rows_mean(const float* x, long d, const long* rows_dev, int n, float* out, hipStream_t s) {
  KtScope kt("rows_mean_kernel", (double)n * (double)d, 4.0 * ((double)n + 1.0) * (double)d, s);
  hipLaunchKernelGGL(rows_mean_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, x, d, rows_dev, n, out);
}

}  // namespace gr
