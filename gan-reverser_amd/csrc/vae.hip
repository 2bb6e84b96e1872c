// vae.hip — the sampling layer of a variational autoencoder on device tensors (gr_vae_sample_dev, gr_vae_sample_backward_dev; new: no counterpart
// in the reference, whose README asks to "compare to Autoencoders, especially VAEs").  h [B x 2 nd] floats: columns 0 .. nd - 1 of a row are mu,
// columns nd .. 2 nd - 1 are logvar; eps, z, gz [B x nd]; gh [B x 2 nd].
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/vae_oracle.py; this file is compiled without FMA contraction
// (Makefile), so every multiply and add below rounds on its own.  Everything past the loads is fp64: the floats enter by an exact conversion.
// No floating-point atomics, no grid barrier, nothing sized by the CU count: every result is a function of the inputs alone.
//
// Operation by operation (all fp64, exp the device library's):
//   forward    s = exp(0.5 * lv);  se = s * eps;  z = (float)(mu + se)
//              element KL: mm = mu * mu, ss = s * s, a = mm + ss, b = a - 1, d = b - lv, k = 0.5 * d
//              kl_rows[i] = (float)K_i, K_i = the k of row i added in column order from +0.0
//              kl[0]: per block of 512 consecutive rows the K_i in row order from +0.0, the block partials in block order from +0.0, one division by B
//   backward   c = kl_weight / B (formed on the host: one fp64 division);  s = exp(0.5 * lv), the same bits as forward's
//              gmu = (float)(gz + c * mu)
//              glv = (float)((gz * eps) * (0.5 * s) + c * (0.5 * (s * s - 1)))
//   a null eps is eps = 0 in both.
//
// Kernels:
//   vae_sample_kernel<VEC>            workgroup = VS_TR rows; thread = one element (VEC: four, 16-byte loads and stores); the element KLs go to LDS, then
//                                     thread = row adds its row in column order.  The chain is serial by contract: a shuffle tree would change the bits
//   (chain.hip, launch_chain_mean)    kl[0] from the K_i
//   vae_sample_backward_kernel<VEC>   thread = one element (VEC: four), grid-stride
// This is a bandwidth-bound layer: 12 nd B bytes in, 4 nd B out, forward; 16 nd B in, 8 nd B out, backward.
#include "kernels.h"

namespace gr {

constexpr int VS_TR = 8;                // rows per workgroup of the forward kernel
constexpr int VS_MAX = 256;             // nd at most

__device__ __forceinline__ void vs_forward_elem(float mu_f, float lv_f, float ep_f, float& z, double& k) {
  const double mu = (double)mu_f, lv = (double)lv_f, ep = (double)ep_f;
  const double s = exp(0.5 * lv);
  const double se = s * ep;
  z = (float)(mu + se);
  const double mm = mu * mu;
  const double ss = s * s;
  const double a = mm + ss;
  const double b = a - 1.0;
  const double d = b - lv;
  k = 0.5 * d;
}

template <bool VEC>
__global__ __launch_bounds__(256) void vae_sample_kernel(const float* __restrict__ h, const float* __restrict__ eps, long B, int nd, float* __restrict__ z,
                                                          float* __restrict__ kl_rows, double* __restrict__ rowkl) {
  __shared__ double ks[VS_TR][VS_MAX + 1];                               // odd pitch: the row threads read distinct banks
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * VS_TR;
  const int nr = (int)min((long)VS_TR, B - r0);
  const bool want = kl_rows != nullptr || rowkl != nullptr;              // (the same in every thread)
  if (VEC) {
    const int nq = nd >> 2;
    for (int e = tid; e < nr * nq; e += 256) {
      const int r = e / nq, c = (e - r * nq) * 4;
      const long row = r0 + r;
      const float4 m = *reinterpret_cast<const float4*>(h + row * 2 * nd + c);
      const float4 l = *reinterpret_cast<const float4*>(h + row * 2 * nd + nd + c);
      const float4 p = eps ? *reinterpret_cast<const float4*>(eps + row * nd + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float mv[4] = {m.x, m.y, m.z, m.w}, lv[4] = {l.x, l.y, l.z, l.w}, pv[4] = {p.x, p.y, p.z, p.w};
      float zv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        double k;
        vs_forward_elem(mv[u], lv[u], pv[u], zv[u], k);
        if (want) ks[r][c + u] = k;
      }
      *reinterpret_cast<float4*>(z + row * nd + c) = make_float4(zv[0], zv[1], zv[2], zv[3]);
    }
  } else {
    for (int e = tid; e < nr * nd; e += 256) {
      const int r = e / nd, c = e - r * nd;
      const long row = r0 + r;
      float zv;
      double k;
      vs_forward_elem(h[row * 2 * nd + c], h[row * 2 * nd + nd + c], eps ? eps[row * nd + c] : 0.f, zv, k);
      z[row * nd + c] = zv;
      if (want) ks[r][c] = k;
    }
  }
  if (!want) return;
  __syncthreads();
  if (tid < nr) {
    double s = 0.0;
    for (int t = 0; t < nd; ++t) s = s + ks[tid][t];
    if (kl_rows) kl_rows[r0 + tid] = (float)s;
    if (rowkl) rowkl[r0 + tid] = s;
  }
}

__device__ __forceinline__ void vs_backward_elem(float mu_f, float lv_f, float ep_f, float gz_f, double c, float& gmu, float& glv) {
  const double mu = (double)mu_f, lv = (double)lv_f, ep = (double)ep_f, gz = (double)gz_f;
  const double s = exp(0.5 * lv);
  const double cm = c * mu;
  gmu = (float)(gz + cm);
  const double ge = gz * ep;
  const double hs = 0.5 * s;
  const double t1 = ge * hs;
  const double ss = s * s;
  const double sm = ss - 1.0;
  const double hm = 0.5 * sm;
  const double t2 = c * hm;
  glv = (float)(t1 + t2);
}

template <bool VEC>
__global__ __launch_bounds__(256) void vae_sample_backward_kernel(const float* __restrict__ h, const float* __restrict__ eps, const float* __restrict__ gz,
                                                                   long B, int nd, double c, float* __restrict__ gh) {
  const int per = VEC ? nd >> 2 : nd;                                    // threads' items per row
  const long total = B * per, stride = (long)gridDim.x * 256;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const long row = e / per;
    const int q = (int)(e - row * per);
    if (VEC) {
      const int col = q * 4;
      const float4 m = *reinterpret_cast<const float4*>(h + row * 2 * nd + col);
      const float4 l = *reinterpret_cast<const float4*>(h + row * 2 * nd + nd + col);
      const float4 p = eps ? *reinterpret_cast<const float4*>(eps + row * nd + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 g = *reinterpret_cast<const float4*>(gz + row * nd + col);
      const float mv[4] = {m.x, m.y, m.z, m.w}, lv[4] = {l.x, l.y, l.z, l.w}, pv[4] = {p.x, p.y, p.z, p.w}, gv[4] = {g.x, g.y, g.z, g.w};
      float a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) vs_backward_elem(mv[u], lv[u], pv[u], gv[u], c, a[u], b[u]);
      *reinterpret_cast<float4*>(gh + row * 2 * nd + col) = make_float4(a[0], a[1], a[2], a[3]);
      *reinterpret_cast<float4*>(gh + row * 2 * nd + nd + col) = make_float4(b[0], b[1], b[2], b[3]);
    } else {
      float a, b;
      vs_backward_elem(h[row * 2 * nd + q], h[row * 2 * nd + nd + q], eps ? eps[row * nd + q] : 0.f, gz[row * nd + q], c, a, b);
      gh[row * 2 * nd + q] = a;
      gh[row * 2 * nd + nd + q] = b;
    }
  }
}

// ------------------------------------------------------------------ launchers
int launch_vae_sample(const float* h, const float* eps, long B, int nd, float* z, float* kl_rows, double* kl, void* workspace, hipStream_t s) {
  if (B < 1 || B > 0x7FFFFFFFL || nd < 1 || nd > VS_MAX) return 1;
  double* rowkl = kl ? reinterpret_cast<double*>(workspace) : nullptr;
  const bool vec = nd % 4 == 0 && aligned16(h) && aligned16(z) && (!eps || aligned16(eps));
  const unsigned grid = (unsigned)((B + VS_TR - 1) / VS_TR);
  { KtScope kt("vae_sample_kernel", 12.0 * B * nd, 16.0 * B * nd, s);
    if (vec) hipLaunchKernelGGL(vae_sample_kernel<true>, dim3(grid), dim3(256), 0, s, h, eps, B, nd, z, kl_rows, rowkl);
    else hipLaunchKernelGGL(vae_sample_kernel<false>, dim3(grid), dim3(256), 0, s, h, eps, B, nd, z, kl_rows, rowkl); }
  if (kl) launch_chain_mean(rowkl, B, rowkl + (size_t)B, kl, "vae_kl_kernels", s);      // workspace: K [B], then the block partials
  return 0;
}

int launch_vae_sample_backward(const float* h, const float* eps, const float* gz, long B, int nd, double c, float* gh, hipStream_t s) {
  if (B < 1 || B > 0x7FFFFFFFL || nd < 1 || nd > VS_MAX) return 1;
  const bool vec = nd % 4 == 0 && aligned16(h) && aligned16(gz) && aligned16(gh) && (!eps || aligned16(eps));
  const long items = B * (vec ? nd >> 2 : nd);
  const long blocks = (items + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
  KtScope kt("vae_sample_backward_kernel", 12.0 * B * nd, 24.0 * B * nd, s);
  if (vec) hipLaunchKernelGGL(vae_sample_backward_kernel<true>, dim3(grid), dim3(256), 0, s, h, eps, gz, B, nd, c, gh);
  else hipLaunchKernelGGL(vae_sample_backward_kernel<false>, dim3(grid), dim3(256), 0, s, h, eps, gz, B, nd, c, gh);
  return 0;
}

}  // namespace gr
