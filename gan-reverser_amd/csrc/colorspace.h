// colorspace.h - the per-pixel arithmetic of NN_UTILS.toRgb / rgbToColorSpace (utils/nn_utils.lua:133-246) as device functions, shared by
// colorspace_kernel* (elem.hip) and the image-grid kernels (render.hip) so that both run the same instructions.  Every file that includes
// this is compiled with -ffp-contract=off: each operation below is one IEEE fp32 operation and `/` is the correctly rounded division.
// max / min are compare-selects, not v_max_f32 / v_min_f32: the result for (+0, -0) is then the one the operation order states.
#pragma once
#include "kernels.h"

namespace gr {

struct Px3 { float a, b, c; };
constexpr float CS_1_3 = 1.0f / 3.0f, CS_1_6 = 1.0f / 6.0f, CS_2_3 = 2.0f / 3.0f;      // rounded to fp32 once
__device__ __forceinline__ float cs_hue(float p, float q, float t) {
  if (t < 0.f) t = t + 1.f;
  if (t > 1.f) t = t - 1.f;
  if (t < CS_1_6) return p + ((q - p) * 6.f) * t;
  if (t < 0.5f) return q;
  if (t < CS_2_3) return p + ((q - p) * (CS_2_3 - t)) * 6.f;
  return p;
}
template <int FROM>
__device__ __forceinline__ Px3 cs_to_rgb(Px3 x) {
  if (FROM == CS_Y) return Px3{x.a, x.a, x.a};                          // torch.repeatTensor(images, 1, 3, 1, 1)
  if (FROM == CS_YUV) {
    Px3 o;
    o.a = x.a + 1.13983f * x.c;
    o.b = (x.a - 0.39465f * x.b) - 0.58060f * x.c;
    o.c = x.a + 2.03211f * x.b;
    return o;
  }
  if (FROM == CS_HSL) {
    const float h = x.a, s = x.b, l = x.c;
    if (s == 0.f) return Px3{l, l, l};
    const float q = l < 0.5f ? l * (1.f + s) : (l + s) - l * s;
    const float p = 2.f * l - q;
    return Px3{cs_hue(p, q, h + CS_1_3), cs_hue(p, q, h), cs_hue(p, q, h - CS_1_3)};
  }
  return x;
}
template <int TO>
__device__ __forceinline__ Px3 cs_from_rgb(Px3 x) {
  const float r = x.a, g = x.b, b = x.c;
  if (TO == CS_Y) return Px3{((0.f + 0.21f * r) + 0.72f * g) + 0.07f * b, 0.f, 0.f};      // z:add(0.21, r):add(0.72, g):add(0.07, b)
  if (TO == CS_YUV) {
    Px3 o;
    o.a = ((0.f + 0.299f * r) + 0.587f * g) + 0.114f * b;
    o.b = ((0.f - 0.14713f * r) - 0.28886f * g) + 0.436f * b;
    o.c = ((0.f + 0.615f * r) - 0.51499f * g) - 0.10001f * b;
    return o;
  }
  if (TO == CS_HSL) {
    float mx = r > g ? r : g; mx = mx > b ? mx : b;
    float mn = r < g ? r : g; mn = mn < b ? mn : b;
    if (mx == mn) return Px3{0.f, 0.f, mx};
    const float d = mx - mn;
    const float l = (mx + mn) / 2.f;
    const float s = l > 0.5f ? d / ((2.f - mx) - mn) : d / (mx + mn);
    float h;
    if (mx == r) h = (g - b) / d + (g < b ? 6.f : 0.f);
    else if (mx == g) h = (b - r) / d + 2.f;
    else h = (r - g) / d + 4.f;
    return Px3{h / 6.f, s, l};
  }
  return x;
}

}  // namespace gr
