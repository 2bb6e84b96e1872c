// dataset.hip — dataset.lua's per-image work where the images will live: image.scale (bilinear) and the loader's fused
// bytes -> [0, 1] -> scale -> rgbToColorSpace [-> NN_UTILS.normalize] path.
// Compiled with -ffp-contract=off: every value below is produced by single IEEE fp32 operations in the order include/ganrev.h states
// (gr_image_scale_dev, gr_dataset_images_dev), `/` is the correctly rounded division, nothing is re-associated, so
// tests/dataset_oracle.py matches these kernels bit for bit.
//
// Replaces (reference file:line):
//   image.load(fp, 3, "float")                              dataset.lua:111,149   (the decoded bytes / 255, grey replicated, alpha dropped)
//   image.scale(img, width, height)                         dataset.lua:112,150
//   NN_UTILS.rgbToColorSpace(images, colorSpace)            dataset.lua:116,153   (the device functions of colorspace.h)
//   NN_UTILS.normalize                                      utils/nn_utils.lua:371-375
//
// The scale arithmetic restates the un-vendored `image` rock's scaleBilinear (generic/image.c: scaleLinear_rowcol, rows first, then
// columns) from memory, like the yuv / hsl arithmetic of colorspace.h: it is unpinned.
//
// Shape: one thread computes PX (1 or 4) adjacent output pixels of every plane.  It walks the vertical source span of its output row and,
// for each source row of the span, evaluates the row-pass value in registers - the fp32 intermediate of the two-pass algorithm is rounded
// where the row pass would round it but never written.  Grid-stride loop over a bounded grid, no LDS.  The _v4 forms store 16 bytes per
// plane and (dataset kernel) read the interleaved bytes as aligned dwords; the scalar forms take any width and any alignment.  The gather
// kernel at the end of the file is the dataset kernel over a cache of images of mixed size: one launch for any list of them.
#include "kernels.h"
#include "colorspace.h"

namespace gr {

// what one output index of a pass reads: kind 0 = src[i0]; 1 = (1 - f0) src[i0] + f0 src[i0 + 1]; 2 = the fractional box [i0 + f0, i1 + f1)
struct ScaleSpan { int i0, i1; float f0, f1; int kind; };
template <int NC> struct Vals { float v[NC]; };

__device__ __forceinline__ ScaleSpan scale_span(const ScaleAxis& a, int di) {
  ScaleSpan s{di, 0, 0.f, 0.f, 0};
  if (a.mode == SCALE_COPY) return s;
  if (a.mode == SCALE_REPLICATE) { s.i0 = 0; return s; }
  if (a.mode == SCALE_UP) {
    if (di == a.dst_len - 1) { s.i0 = a.src_len - 1; return s; }
    float f = (float)di * a.scale;
    const int i = (int)f;                                 // i <= src_len - 2: di <= dst_len - 2 and the lengths are at most 2^15 (launch_* callers check)
    f = f - (float)i;
    s.i0 = i; s.f0 = f; s.kind = 1;
    return s;
  }
  // the recurrence's state before output di is the split of (float)di * scale: the closed form of (i0, f0) = previous (i1, f1)
  float f0 = (float)di * a.scale;
  const int i0 = (int)f0;
  f0 = f0 - (float)i0;
  float f1 = (float)(di + 1) * a.scale;
  const int i1 = (int)f1;                                 // i1 <= src_len for the same reason
  f1 = f1 - (float)i1;
  s.i0 = i0; s.i1 = i1; s.f0 = f0; s.f1 = f1; s.kind = 2;
  return s;
}

// scaleLinear_rowcol for one output index: fetch(i) yields source element i (NC channels side by side)
template <int NC, class Fetch>
__device__ __forceinline__ Vals<NC> span_eval(const ScaleSpan& s, int src_len, Fetch fetch) {
  Vals<NC> acc = fetch(s.i0);
  if (s.kind == 0) return acc;
  if (s.kind == 1) {
    const Vals<NC> b = fetch(s.i0 + 1);
    const float w = 1.f - s.f0;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc.v[c] = w * acc.v[c] + s.f0 * b.v[c];
    return acc;
  }
  float n = 1.f - s.f0;
#pragma unroll
  for (int c = 0; c < NC; ++c) acc.v[c] = n * acc.v[c];
  for (int t = s.i0 + 1; t < s.i1; ++t) {
    const Vals<NC> b = fetch(t);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc.v[c] = acc.v[c] + b.v[c];
    n = n + 1.f;
  }
  if (s.i1 < src_len) {
    const Vals<NC> b = fetch(s.i1);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc.v[c] = acc.v[c] + s.f1 * b.v[c];
    n = n + s.f1;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) acc.v[c] = acc.v[c] / n;
  return acc;
}

// output pixel of the two passes: the column pass over row-pass values, each evaluated (and rounded) on the fly
template <int NC, class Pixel>
__device__ __forceinline__ Vals<NC> scaled_pixel(const ScaleAxis& ay, const ScaleAxis& ax, const ScaleSpan& sy, const ScaleSpan& sx, Pixel pixel) {
  return span_eval<NC>(sy, ay.src_len, [&](int y) { return span_eval<NC>(sx, ax.src_len, [&](int x) { return pixel(y, x); }); });
}

// ------------------------------------------------------------------ image.scale on fp32 planes [nplanes x sh x sw] -> [nplanes x dh x dw]
template <int PX>
__global__ __launch_bounds__(256) void image_scale_kernel(const float* __restrict__ in, float* __restrict__ out, long nplanes, ScaleAxis ay, ScaleAxis ax) {
  const int groups = ax.dst_len / PX;                     // PX == 4: dst_len % 4 == 0
  const long total = nplanes * ay.dst_len * groups;
  const long plane_in = (long)ay.src_len * ax.src_len;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long row = p / groups;                          // plane * dh + dy
    const int gx = (int)(p - row * groups);
    const long plane = row / ay.dst_len;
    const int dy = (int)(row - plane * ay.dst_len);
    const float* src = in + plane * plane_in;
    const ScaleSpan sy = scale_span(ay, dy);
    float r[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j)
      r[j] = scaled_pixel<1>(ay, ax, sy, scale_span(ax, gx * PX + j), [&](int y, int x) { return Vals<1>{{src[(long)y * ax.src_len + x]}}; }).v[0];
    float* dst = out + row * ax.dst_len + gx * PX;
    if constexpr (PX == 4) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    else dst[0] = r[0];
  }
}

void launch_image_scale(const float* in, long nplanes, const ScaleAxis& ay, const ScaleAxis& ax, float* out, hipStream_t s) {
  const bool v4 = ax.dst_len % 4 == 0 && aligned16(out);
  const long npix = nplanes * ay.dst_len * ax.dst_len;
  const long work = v4 ? npix / 4 : npix;
  long blocks = (work + 255) / 256; if (blocks > 2048) blocks = 2048;
  KtScope kt(v4 ? "image_scale_kernel_v4" : "image_scale_kernel", 0.0, 4.0 * ((double)nplanes * ay.src_len * ax.src_len + (double)npix), s);
  if (v4) hipLaunchKernelGGL((image_scale_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, s, in, out, nplanes, ay, ax);
  else hipLaunchKernelGGL((image_scale_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, s, in, out, nplanes, ay, ax);
}

// ------------------------------------------------------------------ the loader's fused path: uint8 HWC [n x sh x sw x SC] -> fp32 NCHW [n x CO x dh x dw]
// V4: PX = 4, 16-byte stores, and the bytes of a pixel come from aligned dwords (SC 4: one; SC 3: the one or two that hold them, funnel-shifted;
// the launcher checks that `in` is 4-byte aligned and that the tensor ends on a dword boundary, so every such dword lies inside it).
template <int SC, bool V4>
__device__ __forceinline__ Vals<(SC == 1 ? 1 : 3)> load_pixel(const uint8_t* __restrict__ in, long pix) {
  constexpr float K = 255.0f;
  if constexpr (SC == 1) {
    return Vals<1>{{(float)in[pix] / K}};
  } else {
    unsigned w;
    if constexpr (!V4) {
      const uint8_t* p = in + pix * SC;
      w = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    } else if constexpr (SC == 4) {
      w = reinterpret_cast<const unsigned*>(in)[pix];
    } else {
      const long o = pix * 3;
      const unsigned* q = reinterpret_cast<const unsigned*>(in) + (o >> 2);
      const unsigned sh = (unsigned)o & 3u;
      const unsigned lo = q[0];
      const unsigned hi = sh >= 2u ? q[1] : 0u;           // the pixel's third byte lies in the next dword
      w = (unsigned)((((unsigned long long)hi << 32) | lo) >> (8u * sh));
    }
    return Vals<3>{{(float)(w & 255u) / K, (float)((w >> 8) & 255u) / K, (float)((w >> 16) & 255u) / K}};
  }
}

__device__ __forceinline__ float normalize_value(float v) {          // utils/nn_utils.lua:372-374
  v = v * 2.f;
  v = v + (-1.f);
  v = v < -1.f ? -1.f : v;
  return v > 1.f ? 1.f : v;
}

// PX adjacent output pixels (row dy, columns gx * PX ...) of the image whose pixels start at pixel `base` of `in`: the two scale passes over
// load_pixel<SC, DW>, the colour space, the normalise step.  The per-pixel body of both kernels below.
template <int SC, int TO, int PX, bool DW>
__device__ __forceinline__ void dataset_pixels(const uint8_t* __restrict__ in, long base, const ScaleAxis& ay, const ScaleAxis& ax, int dy, int gx, int normalize, Px3 (&y)[PX]) {
  constexpr int NC = SC == 1 ? 1 : 3, CO = TO == CS_Y ? 1 : 3;
  const ScaleSpan sy = scale_span(ay, dy);
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    const Vals<NC> v = scaled_pixel<NC>(ay, ax, sy, scale_span(ax, gx * PX + j),
                                        [&](int yy, int xx) { return load_pixel<SC, DW>(in, base + (long)yy * ax.src_len + xx); });
    Px3 rgb{v.v[0], v.v[0], v.v[0]};                    // grey: the plane three times
    if constexpr (NC == 3) { rgb.b = v.v[1]; rgb.c = v.v[2]; }
    y[j] = cs_from_rgb<TO>(rgb);
    if (normalize) { y[j].a = normalize_value(y[j].a); if (CO == 3) { y[j].b = normalize_value(y[j].b); y[j].c = normalize_value(y[j].c); } }
  }
}
// ... and their store: PX == 4 writes 16 bytes per plane (dst 16-byte aligned), PX == 1 one float
template <int TO, int PX>
__device__ __forceinline__ void store_pixels(float* __restrict__ dst, long plane_out, const Px3 (&y)[PX]) {
  constexpr int CO = TO == CS_Y ? 1 : 3;
  if constexpr (PX == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(y[0].a, y[1].a, y[2].a, y[3].a);
    if (CO == 3) {
      *reinterpret_cast<float4*>(dst + plane_out) = make_float4(y[0].b, y[1].b, y[2].b, y[3].b);
      *reinterpret_cast<float4*>(dst + 2 * plane_out) = make_float4(y[0].c, y[1].c, y[2].c, y[3].c);
    }
  } else {
    dst[0] = y[0].a;
    if (CO == 3) { dst[plane_out] = y[0].b; dst[2 * plane_out] = y[0].c; }
  }
}

template <int SC, int TO, bool V4>
__global__ __launch_bounds__(256) void dataset_images_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, long n, ScaleAxis ay, ScaleAxis ax, int normalize) {
  constexpr int PX = V4 ? 4 : 1, CO = TO == CS_Y ? 1 : 3;
  const int groups = ax.dst_len / PX;
  const long total = n * ay.dst_len * groups;
  const long image_in = (long)ay.src_len * ax.src_len, plane_out = (long)ay.dst_len * ax.dst_len;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long row = p / groups;                          // image * dh + dy
    const int gx = (int)(p - row * groups);
    const long img = row / ay.dst_len;
    const int dy = (int)(row - img * ay.dst_len);
    Px3 y[PX];
    dataset_pixels<SC, TO, PX, V4>(in, img * image_in, ay, ax, dy, gx, normalize, y);
    store_pixels<TO, PX>(out + img * CO * plane_out + (long)dy * ax.dst_len + gx * PX, plane_out, y);
  }
}

template <int SC, int TO>
static void dataset_launch(const uint8_t* in, long n, const ScaleAxis& ay, const ScaleAxis& ax, int normalize, float* out, hipStream_t s) {
  const double bytes_in = (double)n * ay.src_len * ax.src_len * SC;
  const long npix = n * ay.dst_len * ax.dst_len;
  // 16-byte stores need whole groups of four per output row (then every plane row starts 16-byte aligned when `out` does); dword reads of the
  // bytes need `in` dword aligned and a tensor that ends on a dword boundary
  const bool v4 = ax.dst_len % 4 == 0 && aligned16(out) && ((uintptr_t)in & 3) == 0 && ((long)bytes_in & 3) == 0;
  const long work = v4 ? npix / 4 : npix;
  long blocks = (work + 255) / 256; if (blocks > 2048) blocks = 2048;
  KtScope kt(v4 ? "dataset_images_kernel_v4" : "dataset_images_kernel", 0.0, bytes_in + 4.0 * (TO == CS_Y ? 1 : 3) * (double)npix, s);
  if (v4) hipLaunchKernelGGL((dataset_images_kernel<SC, TO, true>), dim3((unsigned)blocks), dim3(256), 0, s, in, out, n, ay, ax, normalize);
  else hipLaunchKernelGGL((dataset_images_kernel<SC, TO, false>), dim3((unsigned)blocks), dim3(256), 0, s, in, out, n, ay, ax, normalize);
}
template <int SC>
static void dataset_launch_to(const uint8_t* in, long n, const ScaleAxis& ay, const ScaleAxis& ax, int to, int normalize, float* out, hipStream_t s) {
  switch (to) {
    case CS_RGB: dataset_launch<SC, CS_RGB>(in, n, ay, ax, normalize, out, s); break;
    case CS_Y: dataset_launch<SC, CS_Y>(in, n, ay, ax, normalize, out, s); break;
    case CS_YUV: dataset_launch<SC, CS_YUV>(in, n, ay, ax, normalize, out, s); break;
    default: dataset_launch<SC, CS_HSL>(in, n, ay, ax, normalize, out, s); break;
  }
}
void launch_dataset_images(const uint8_t* in, long n, int sc, const ScaleAxis& ay, const ScaleAxis& ax, int to, int normalize, float* out, hipStream_t s) {
  switch (sc) {
    case 1: dataset_launch_to<1>(in, n, ay, ax, to, normalize, out, s); break;
    case 3: dataset_launch_to<3>(in, n, ay, ax, to, normalize, out, s); break;
    default: dataset_launch_to<4>(in, n, ay, ax, to, normalize, out, s); break;
  }
}

// ------------------------------------------------------------------ the same over a cache of decoded files (gr_dataset_cache_load_dev)
// Row k of out is image recs[idx[k]] at ITS source size and channel count: the record is read once per item, its two ScaleAxis are built by
// the function the host builds them with (one correctly rounded division each), the channel count is a branch (uniform over a wave wherever a
// wave stays inside one image: always at dh * dw / PX >= 64 items per image).  Every cached image is read in load_pixel's dword form - the
// cache places it on a 4-byte boundary, pads it to a dword and keeps a dword of the allocation behind it; V4 here is the store form alone.
template <int TO, bool V4>
__global__ __launch_bounds__(256) void dataset_gather_kernel(const CachedImage* __restrict__ recs, const long* __restrict__ idx, float* __restrict__ out, long n, int dh, int dw,
                                                             int normalize) {
  constexpr int PX = V4 ? 4 : 1, CO = TO == CS_Y ? 1 : 3;
  const int groups = dw / PX;
  const long total = n * dh * groups;
  const long plane_out = (long)dh * dw;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long row = p / groups;                          // k * dh + dy
    const int gx = (int)(p - row * groups);
    const long k = row / dh;
    const int dy = (int)(row - k * dh);
    const CachedImage im = recs[idx[k]];
    const ScaleAxis ay = scale_axis(im.sh, dh), ax = scale_axis(im.sw, dw);
    Px3 y[PX];
    if (im.sc == 3) dataset_pixels<3, TO, PX, true>(im.data, 0, ay, ax, dy, gx, normalize, y);
    else if (im.sc == 4) dataset_pixels<4, TO, PX, true>(im.data, 0, ay, ax, dy, gx, normalize, y);
    else dataset_pixels<1, TO, PX, true>(im.data, 0, ay, ax, dy, gx, normalize, y);
    store_pixels<TO, PX>(out + k * CO * plane_out + (long)dy * dw + gx * PX, plane_out, y);
  }
}

template <int TO>
static void gather_launch(const CachedImage* recs, const long* idx, long n, int dh, int dw, int normalize, float* out, double bytes_in, hipStream_t s) {
  const long npix = n * dh * dw;
  const bool v4 = dw % 4 == 0 && aligned16(out);      // whole groups of four per output row: every plane row then starts 16-byte aligned when `out` does
  const long work = v4 ? npix / 4 : npix;
  long blocks = (work + 255) / 256; if (blocks > 2048) blocks = 2048;
  KtScope kt(v4 ? "dataset_gather_kernel_v4" : "dataset_gather_kernel", 0.0, bytes_in + 4.0 * (TO == CS_Y ? 1 : 3) * (double)npix, s);
  if (v4) hipLaunchKernelGGL((dataset_gather_kernel<TO, true>), dim3((unsigned)blocks), dim3(256), 0, s, recs, idx, out, n, dh, dw, normalize);
  else hipLaunchKernelGGL((dataset_gather_kernel<TO, false>), dim3((unsigned)blocks), dim3(256), 0, s, recs, idx, out, n, dh, dw, normalize);
}
void launch_dataset_gather(const CachedImage* recs, const long* idx, long n, int dh, int dw, int to, int normalize, float* out, double bytes_in, hipStream_t s) {
  switch (to) {
    case CS_RGB: gather_launch<CS_RGB>(recs, idx, n, dh, dw, normalize, out, bytes_in, s); break;
    case CS_Y: gather_launch<CS_Y>(recs, idx, n, dh, dw, normalize, out, bytes_in, s); break;
    case CS_YUV: gather_launch<CS_YUV>(recs, idx, n, dh, dw, normalize, out, bytes_in, s); break;
    default: gather_launch<CS_HSL>(recs, idx, n, dh, dw, normalize, out, bytes_in, s); break;
  }
}

}  // namespace gr
