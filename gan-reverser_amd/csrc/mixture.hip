// mixture.hip — a diagonal-covariance Gaussian mixture of a device table [n x d] fitted by EM, d <= 256, k <= 256 (gr_mixture_dev; new: no
// counterpart in the reference, whose README asks for "other clustering methods").
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/mixture_paths.py; this file is compiled without FMA contraction
// (Makefile), so every multiply and add below rounds on its own.  Everything past the loads is fp64: x, the means, the variances and the weights
// are floats and enter by an exact conversion.  No floating-point atomics, no grid barrier: every result is a function of the inputs alone.
//
// Operation by operation (all fp64, exp and log the device library's):
//   per component, once per E-step  h_jt = 0.5 / var_jt;  c_j = log(w_j) - 0.5 * (d * log(2 pi) + S_j), S_j = the log(var_jt) added in column order
//                                   from +0.0
//   log-density                     dl = x_it - mu_jt;  e = dl * dl;  q = q + e * h_jt in column order from +0.0;  l_ij = c_j - q
//   row log-likelihood              components are split into 4 contiguous ranges of ceil(k / 4); within a range in ascending j the running pair
//                                   (m, s) from (-inf, 0):  l > m: s = s * exp(m - l) + 1, m = l, label = j;  otherwise, for l > -inf:
//                                   s = s + exp(l - m).  Then M = the largest m (the lowest range among equals), S = the s_g * exp(m_g - M) added
//                                   in range order from +0.0, L_i = M + log(S); label = that range's; post = (float)exp(M - L_i); rowll = (float)L_i
//   mean log-likelihood             per block of 512 rows the L_i in row order from +0.0, the block partials in block order from +0.0, one division by n
//   responsibilities                r_ij = exp(l_ij - L_i) with l_ij recomputed by the chain above (the same bits), 0 where l_ij = -inf
//   M-step sums                     per block of 512 rows and (j, t) three chains in row order from +0.0:  a1 = a1 + r * x;  dl = x - mu_jt,
//                                   e = dl * dl, a2 = a2 + r * e;  an = an + r.  MX_P = 128 partial sets, set p adding the chains of the blocks
//                                   floor(p B / P) .. floor((p + 1) B / P) - 1 in block order from +0.0; the sets added in order from +0.0
//   update                          N_j >= 1:  mu' = S1 / N;  dm = mu' - mu;  var' = S2 / N - dm * dm, var_floor where that is not above it; both
//                                   rounded to float once;  w' = (float)(N / n) always
//
// Kernels:
//   mix_prep_kernel          thread = component
//   mix_estep_kernel         workgroup = 64 rows held in LDS, wave = one of the 4 component ranges (means and h through the scalar cache), lane = row
//   (chain.hip, launch_chain_mean)  loglik[it] from the L_i
//   mix_mstep_kernel         workgroup = (8 components, one of the MX_P block ranges); per stage of 64 rows: r for the 64 x 8 pairs (lane = row,
//                            wave = 2 components) into LDS, then thread = (column, JPT of the 8 components) adds the stage's rows in row order.
//                            JPT = 8, 4, 2, 1 for d <= 256, 128, 64, 32, so that narrow tables still fill the workgroup
//   mix_update_kernel        workgroup = component, thread = column
// The E-step and the M-step do not share a launch: L_i must be known before the first r_ij, and r [n x k] is never stored (scratch stays O(n)):
// the M-step recomputes l_ij, which costs 4 of the iteration's 15 fp64 operations per (row, component, column).
#include "kernels.h"

namespace gr {

constexpr int MX_P = 128;               // partial sets of the M-step sums: a constant of the library (tests/mixture_paths.py restates it)
constexpr int MX_TR = 64;               // rows per LDS stage
constexpr int MX_JT = 8;                // components per M-step workgroup
constexpr int MX_MAX = 256;             // columns and components at most
constexpr double MX_LOG_2PI = 1.8378770664093454835606594728112;

__global__ void mix_prep_kernel(const float* __restrict__ w, const float* __restrict__ vars, int k, int d, double* __restrict__ cst, double* __restrict__ hinv) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  double s = 0.0;
  for (int t = 0; t < d; ++t) {
    const double v = (double)vars[(long)j * d + t];
    s += log(v);
    hinv[(long)j * d + t] = 0.5 / v;
  }
  cst[j] = log((double)w[j]) - 0.5 * ((double)d * MX_LOG_2PI + s);
}

// l_ij: the chain of the file header.  mj, hj and c are wave-uniform.
__device__ __forceinline__ double mix_logdens(const float* xr, const float* __restrict__ mj, const double* __restrict__ hj, double c, int d) {
  double q = 0.0;
#pragma unroll 4
  for (int t = 0; t < d; ++t) {
    const double dl = (double)xr[t] - (double)mj[t];
    const double e = dl * dl;
    q = q + e * hj[t];
  }
  return c - q;
}

__global__ __launch_bounds__(256) void mix_estep_kernel(const float* __restrict__ x, long n, int d, int k, const float* __restrict__ mu,
                                                         const double* __restrict__ hinv, const double* __restrict__ cst, double* __restrict__ rowl,
                                                         int* __restrict__ labels, float* __restrict__ post, float* __restrict__ rowll) {
  extern __shared__ __attribute__((aligned(16))) float xs[];            // [MX_TR][ld], ld odd: the lanes of a wave read distinct banks
  __shared__ double gm[4][MX_TR], gs[4][MX_TR];
  __shared__ int gi[4][MX_TR];
  const int tid = threadIdx.x, r = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ld = d | 1;
  const long r0 = (long)blockIdx.x * MX_TR;
  const int nr = (int)min((long)MX_TR, n - r0);
  stage_rows<MX_TR, 1>(x, r0, nr, d, ld, xs, tid);
  __syncthreads();
  const int kq = (k + 3) / 4, j_lo = w * kq, j_hi = min(k, j_lo + kq);
  const float* xr = xs + r * ld;
  double m = -INFINITY, s = 0.0;
  int bi = -1;
  for (int j = j_lo; j < j_hi; ++j) {
    const double l = mix_logdens(xr, mu + (long)j * d, hinv + (long)j * d, cst[j], d);
    if (l > m) { s = s * exp(m - l) + 1.0; m = l; bi = j; }
    else if (l > -INFINITY) s = s + exp(l - m);                         // (a dead component, and a NaN, add nothing)
  }
  gm[w][r] = m; gs[w][r] = s; gi[w][r] = bi;
  __syncthreads();
  if (tid < nr) {
    double M = -INFINITY;
    int idx = -1;
    for (int g = 0; g < 4; ++g)
      if (gi[g][tid] >= 0 && gm[g][tid] > M) { M = gm[g][tid]; idx = gi[g][tid]; }
    double S = 0.0;
    for (int g = 0; g < 4; ++g)
      if (gi[g][tid] >= 0) S = S + gs[g][tid] * exp(gm[g][tid] - M);
    const double L = M + log(S);
    rowl[r0 + tid] = L;
    if (labels) labels[r0 + tid] = idx < 0 ? 0 : idx;
    if (post) post[r0 + tid] = (float)exp(M - L);
    if (rowll) rowll[r0 + tid] = (float)L;
  }
}

// part: s1 [MX_P][k][d], then s2 [MX_P][k][d], then sn [MX_P][k]
template <int JPT>
__global__ __launch_bounds__(256) void mix_mstep_kernel(const float* __restrict__ x, long n, int d, int k, const float* __restrict__ mu,
                                                         const double* __restrict__ hinv, const double* __restrict__ cst, const double* __restrict__ rowl,
                                                         double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float xs[];            // [MX_TR][ld]
  __shared__ __attribute__((aligned(16))) double rs[MX_TR][MX_JT];
  constexpr int G = MX_JT / JPT, W = 256 / G;                           // thread = (column t < W, group g of JPT components)
  const int tid = threadIdx.x, j0 = blockIdx.x * MX_JT, p = blockIdx.y;
  const int ld = d | 1;
  const long nblk = row_blocks(n);
  const long b_lo = p * nblk / MX_P, b_hi = (p + 1) * nblk / MX_P;     // contiguous, uneven ranges; empty ones when nblk < MX_P
  const int r1 = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);    // the role in the r pass: row r1, components 2 w and 2 w + 1 of the tile
  const int t = tid % W, g = tid / W;
  const bool col = t < d;
  double mo[JPT], sum1[JPT], sum2[JPT], sumn[JPT];
#pragma unroll
  for (int u = 0; u < JPT; ++u) {
    const int j = j0 + g * JPT + u;
    mo[u] = (col && j < k) ? (double)mu[(long)j * d + t] : 0.0;
    sum1[u] = sum2[u] = sumn[u] = 0.0;
  }
  for (long b = b_lo; b < b_hi; ++b) {
    double a1[JPT], a2[JPT], an[JPT];                                   // a block begins: its chains start from +0
#pragma unroll
    for (int u = 0; u < JPT; ++u) a1[u] = a2[u] = an[u] = 0.0;
    for (int st = 0; st < ROWS_PER_BLOCK / MX_TR; ++st) {
      const long row0 = b * ROWS_PER_BLOCK + (long)st * MX_TR;
      if (row0 >= n) break;                                             // (the same in every thread)
      const int nr = (int)min((long)MX_TR, n - row0);
      __syncthreads();                                                  // the stage before this one has been read
      stage_rows<MX_TR, 1>(x, row0, nr, d, ld, xs, tid);
      __syncthreads();
      const double Li = r1 < nr ? rowl[row0 + r1] : 0.0;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int jj = 2 * w + u, j = j0 + jj;
        double rv = 0.0;
        if (j < k) {                                                    // (wave-uniform)
          const double l = mix_logdens(xs + r1 * ld, mu + (long)j * d, hinv + (long)j * d, cst[j], d);
          if (r1 < nr && l > -INFINITY) rv = exp(l - Li);
        }
        rs[r1][jj] = rv;
      }
      __syncthreads();
      if (col)
        for (int r = 0; r < nr; ++r) {
          const double xv = (double)xs[r * ld + t];
#pragma unroll
          for (int u = 0; u < JPT; ++u) {
            const double rv = rs[r][g * JPT + u];
            a1[u] = a1[u] + rv * xv;
            const double dl = xv - mo[u];
            const double e = dl * dl;
            a2[u] = a2[u] + rv * e;
            an[u] = an[u] + rv;
          }
        }
    }
#pragma unroll
    for (int u = 0; u < JPT; ++u) { sum1[u] += a1[u]; sum2[u] += a2[u]; sumn[u] += an[u]; }     // the block ends: the blocks in block order
  }
  double* s1 = part + (size_t)p * k * d;
  double* s2 = part + (size_t)MX_P * k * d + (size_t)p * k * d;
  double* sn = part + 2 * (size_t)MX_P * k * d + (size_t)p * k;
#pragma unroll
  for (int u = 0; u < JPT; ++u) {
    const int j = j0 + g * JPT + u;
    if (col && j < k) {
      s1[(long)j * d + t] = sum1[u];
      s2[(long)j * d + t] = sum2[u];
      if (t == 0) sn[j] = sumn[u];
    }
  }
}

__global__ __launch_bounds__(256) void mix_update_kernel(const double* __restrict__ part, long n, int d, int k, float var_floor, float* __restrict__ w,
                                                          float* __restrict__ mu, float* __restrict__ vars) {
  const int j = blockIdx.x, t = threadIdx.x;
  const double* s1 = part;
  const double* s2 = part + (size_t)MX_P * k * d;
  const double* sn = part + 2 * (size_t)MX_P * k * d;
  double N = 0.0;
  for (int p = 0; p < MX_P; ++p) N += sn[(size_t)p * k + j];
  if (t < d && N >= 1.0) {                                              // less than one row's worth (or a NaN): the mean and the variances stay
    double a = 0.0, b = 0.0;
    for (int p = 0; p < MX_P; ++p) { a += s1[((size_t)p * k + j) * d + t]; b += s2[((size_t)p * k + j) * d + t]; }
    const double mn = a / N;
    const double dm = mn - (double)mu[(long)j * d + t];
    const double v = b / N - dm * dm;
    const double fl = (double)var_floor;
    mu[(long)j * d + t] = (float)mn;
    vars[(long)j * d + t] = (float)(v > fl ? v : fl);
  }
  if (t == 0) w[j] = (float)(N / (double)n);
}

// ------------------------------------------------------------------ launcher
// doubles: c [k], h [k][d], L [n], the block partials of L [ceil(n / 512)], the MX_P partial sets [MX_P][k][2 d + 1]
size_t mixture_workspace_bytes(long n, int d, int k) {
  return sizeof(double) * ((size_t)k + (size_t)k * d + chain_mean_doubles(n) + (size_t)MX_P * k * (2 * (size_t)d + 1)) + 1024;
}

int launch_mixture(const float* x, long n, int d, int k, int niter, float var_floor, float* w, float* mu, float* vars, double* loglik, int* labels,
                   float* post, float* rowll, void* workspace, hipStream_t s) {
  if (n < 1 || n > 0x7FFFFFFFL || d < 1 || d > MX_MAX || k < 1 || k > MX_MAX || niter < 0 || !(var_floor > 0.f)) return 1;
  double* cst = reinterpret_cast<double*>(workspace);
  double* hinv = cst + k;
  double* rowl = hinv + (size_t)k * d;
  double* llpart = rowl + (size_t)n;
  double* part = llpart + row_blocks(n);
  const int jpt = d > 128 ? 8 : d > 64 ? 4 : d > 32 ? 2 : 1;
  const void* mstep = jpt == 8 ? reinterpret_cast<const void*>(mix_mstep_kernel<8>) : jpt == 4 ? reinterpret_cast<const void*>(mix_mstep_kernel<4>)
                    : jpt == 2 ? reinterpret_cast<const void*>(mix_mstep_kernel<2>) : reinterpret_cast<const void*>(mix_mstep_kernel<1>);
  const size_t lds = sizeof(float) * MX_TR * (size_t)(d | 1);
  if (lds > 40 * 1024)                                                   // (per device; a host-side setting, cheap to repeat)
    for (const void* f : {reinterpret_cast<const void*>(mix_estep_kernel), mstep})
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * MX_TR * 257)) != hipSuccess) return 2;
  const unsigned egrid = (unsigned)((n + MX_TR - 1) / MX_TR);
  auto estep = [&](int it, bool last) {
    { KtScope kt("mix_prep_kernel", 2.0 * k * d, 12.0 * k * d, s);
      hipLaunchKernelGGL(mix_prep_kernel, dim3((k + 63) / 64), dim3(64), 0, s, w, vars, k, d, cst, hinv); }
    { KtScope kt("mix_estep_kernel", 4.0 * n * d * k, 4.0 * n * d + 8.0 * n, s);
      hipLaunchKernelGGL(mix_estep_kernel, dim3(egrid), dim3(256), lds, s, x, n, d, k, mu, hinv, cst, rowl, last ? labels : nullptr, last ? post : nullptr,
                         last ? rowll : nullptr); }
    launch_chain_mean(rowl, n, llpart, loglik + it, "mix_loglik_kernels", s);
  };
  const dim3 mgrid((k + MX_JT - 1) / MX_JT, MX_P);
  for (int it = 0; it < niter; ++it) {
    estep(it, false);
    { KtScope kt("mix_mstep_kernel", 11.0 * n * d * k, 4.0 * n * d * ((k + MX_JT - 1) / MX_JT) + 8.0 * n, s);
      if (jpt == 8) hipLaunchKernelGGL(mix_mstep_kernel<8>, mgrid, dim3(256), lds, s, x, n, d, k, mu, hinv, cst, rowl, part);
      else if (jpt == 4) hipLaunchKernelGGL(mix_mstep_kernel<4>, mgrid, dim3(256), lds, s, x, n, d, k, mu, hinv, cst, rowl, part);
      else if (jpt == 2) hipLaunchKernelGGL(mix_mstep_kernel<2>, mgrid, dim3(256), lds, s, x, n, d, k, mu, hinv, cst, rowl, part);
      else hipLaunchKernelGGL(mix_mstep_kernel<1>, mgrid, dim3(256), lds, s, x, n, d, k, mu, hinv, cst, rowl, part); }
    KtScope kt("mix_update_kernel", 2.0 * MX_P * k * d, 16.0 * MX_P * k * d, s);
    hipLaunchKernelGGL(mix_update_kernel, dim3(k), dim3(256), 0, s, part, n, d, k, var_floor, w, mu, vars);
  }
  estep(niter, true);
  return 0;
}

}  // namespace gr
