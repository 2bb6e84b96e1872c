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
  switch (g.from) {                                   // uniform over the launch; -1 and CS_RGB copy the channels
    case CS_Y: x = cs_to_rgb<CS_Y>(x); break;
    case CS_YUV: x = cs_to_rgb<CS_YUV>(x); break;
    case CS_HSL: x = cs_to_rgb<CS_HSL>(x); break;
    default: break;
  }
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
