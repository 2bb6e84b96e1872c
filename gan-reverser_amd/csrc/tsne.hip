// tsne.hip — exact (dense) t-SNE of a device table [n x d], n <= GR_TSNE_MAX_N (gr_tsne_*_dev, gr_map_cells_dev; new: no counterpart in the
// reference).
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/tsne_paths.py; this file is compiled without FMA contraction
// (Makefile), so every multiply and add below rounds on its own.  No floating-point atomics, no grid barrier, nothing reads the CU count:
// every result is a function of the inputs alone.
//
// Kernels:
//   tsne_transpose_kernel  x [n][d] -> xt [d][n] in scratch, so that the distance loop below reads along a row of xt
//   tsne_cond_kernel       workgroup = row i, 1024 threads, thread t = the columns j = t + 1024 u (u < 16): D_ij in fp64 in registers, the
//                          bisection on beta with two block sums per step (block_tree_sum, kernels.h: one barrier sequence for both),
//                          p_j|i -> p [i][j] (fp32), beta, info (integer atomics)
//   tsne_symm_kernel       workgroup = the 32 x 32 tile (bi, bj), bi <= bj, and its mirror, through LDS: both entries of a pair from one thread
//   tsne_pass_kernel<KL>   workgroup = 8 consecutive rows of P, 256 threads, thread t = the columns j = t + 256 m of all 8 rows (y_j is loaded
//                          once for them); fp32 up to w, fp64 after; per row and sum: lane chain, wave tree, the 4 waves in order
//   tsne_combine_kernel    every workgroup sums the n row values of Z in one fixed order (the same bits everywhere), thread = row: the gradient
//   tsne_kl_join_kernel    ONE workgroup: the three column sums of the KL pass in the same fixed order -> kl
//   tsne_update_kernel     workgroup = block of 512 rows, thread = element: delta-bar-delta; the block's column sums in row order in fp64
//   tsne_centre_kernel     thread = element: the block partials in block order, one division by n, one subtraction
//   cells_*_kernel         gr_map_cells_dev: bounding box (compare-selects), keys to all ones, one 64-bit integer atomicMin per row, unpack
#include "kernels.h"

namespace gr {

constexpr int TS_CT = 1024, TS_CU = 16;         // threads of the row workgroup x columns per thread = GR_TSNE_MAX_N
constexpr int TS_MAX_N = TS_CT * TS_CU;
constexpr int TS_MAX_TRIES = 50;                // updates of beta at most
constexpr double TS_TOL = 1e-5;                 // |H - log(perplexity)| at which the search stops
constexpr int TS_R = 8, TS_PT = 256;            // rows of P per workgroup, threads

__global__ __launch_bounds__(256) void tsne_transpose_kernel(const float* __restrict__ x, int n, int d, float* __restrict__ xt) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * d) return;
  const size_t k = e / n, j = e - k * n;
  xt[e] = x[j * d + k];
}

__global__ __launch_bounds__(TS_CT) void tsne_cond_kernel(const float* __restrict__ x, const float* __restrict__ xt, int n, int d, double logu,
                                                           float* __restrict__ p, double* __restrict__ beta_out, int* __restrict__ info) {
  __shared__ double ra[2 * TS_CT];                                       // the two planes of block_tree_sum; the first also carries the minimum
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* xi = x + (size_t)i * d;
  double D[TS_CU];
#pragma unroll
  for (int u = 0; u < TS_CU; ++u) D[u] = 0.0;
  for (int k = 0; k < d; ++k) {                                          // D_ij = sum_k ((double)x_ik - (double)x_jk)^2 in column order
    const double a = (double)xi[k];
    const float* col = xt + (size_t)k * n;
#pragma unroll
    for (int u = 0; u < TS_CU; ++u) {
      const int j = tid + u * TS_CT;
      if (j < n) { const double t = a - (double)col[j]; D[u] = D[u] + t * t; }
    }
  }
  double dmin = INFINITY;
#pragma unroll
  for (int u = 0; u < TS_CU; ++u) {
    const int j = tid + u * TS_CT;
    if (j < n && j != i) dmin = fmin(dmin, D[u]);
  }
  __syncthreads();
  ra[tid] = dmin;
  __syncthreads();
  for (int o = TS_CT / 2; o > 0; o >>= 1) {
    if (tid < o) ra[tid] = fmin(ra[tid], ra[tid + o]);
    __syncthreads();
  }
  dmin = ra[0];
#pragma unroll
  for (int u = 0; u < TS_CU; ++u) D[u] = D[u] - dmin;
  // the bisection of van der Maaten's reference code; S and SD are the same bits in every thread, so the control flow is uniform
  double beta = 1.0, bmin = 0.0, bmax = 0.0, S = 1.0;
  bool has_min = false, has_max = false, capped = false;
  int tries = 0;
  for (;;) {
    double v[2] = {0.0, 0.0};                                            // (s, sd)
#pragma unroll
    for (int u = 0; u < TS_CU; ++u) {
      const int j = tid + u * TS_CT;
      if (j < n && j != i) { const double e = exp(-beta * D[u]); v[0] = v[0] + e; v[1] = v[1] + D[u] * e; }
    }
    block_tree_sum<TS_CT, 2>(v, ra, tid);
    const double s = v[0], sd = v[1];
    S = s;
    const double diff = (log(s) + beta * sd / s) - logu;
    if (fabs(diff) <= TS_TOL) break;
    if (tries == TS_MAX_TRIES) { capped = true; break; }
    if (diff > 0.0) { bmin = beta; has_min = true; beta = has_max ? (beta + bmax) / 2.0 : beta * 2.0; }
    else { bmax = beta; has_max = true; beta = has_min ? (beta + bmin) / 2.0 : beta / 2.0; }
    ++tries;
  }
  float* prow = p + (size_t)i * n;
#pragma unroll
  for (int u = 0; u < TS_CU; ++u) {
    const int j = tid + u * TS_CT;
    if (j < n) prow[j] = j == i ? 0.f : (float)(exp(-beta * D[u]) / S);
  }
  if (tid == 0) {
    if (beta_out) beta_out[i] = beta;
    atomicMax(&info[0], tries);                                          // integer atomics: the result does not depend on their order
    if (capped) atomicAdd(&info[1], 1);
  }
}

// p_ij = p_ji = (float)(((double)c_ij + (double)c_ji) / (double)(2 n)), in place: the pair (i, j), (j, i) is read and written by one thread
__global__ __launch_bounds__(256) void tsne_symm_kernel(float* __restrict__ p, int n) {
  __shared__ float As[32][33], Bs[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  const double div = (double)(2 * (long)n);
  for (int r = r0; r < 32; r += 8) {
    const int ia = bi * 32 + r, ja = bj * 32 + c, ib = bj * 32 + r, jb = bi * 32 + c;
    As[r][c] = (ia < n && ja < n) ? p[(size_t)ia * n + ja] : 0.f;
    if (bi != bj) Bs[r][c] = (ib < n && jb < n) ? p[(size_t)ib * n + jb] : 0.f;
  }
  __syncthreads();
  for (int r = r0; r < 32; r += 8) {
    const int ia = bi * 32 + r, ja = bj * 32 + c, ib = bj * 32 + r, jb = bi * 32 + c;
    if (bi == bj) {
      if (ia < n && ja < n) p[(size_t)ia * n + ja] = (float)(((double)As[r][c] + (double)As[c][r]) / div);
    } else {
      if (ia < n && ja < n) p[(size_t)ia * n + ja] = (float)(((double)As[r][c] + (double)Bs[c][r]) / div);
      if (ib < n && jb < n) p[(size_t)ib * n + jb] = (float)(((double)Bs[r][c] + (double)As[c][r]) / div);
    }
  }
}

// One pass over P.  KL == 0: per row the sums (sum_j p w dx, sum_j p w dy, sum_j w^2 dx, sum_j w^2 dy, sum_{j != i} w); KL == 1: per row
// (sum_{p > 0} p (log p - log w), sum_j p, sum_{j != i} w).  dx = y_i0 - y_j0, dy = y_i1 - y_j1, w = 1 / (1 + (dx dx + dy dy)) in fp32, each
// operation rounded; everything after w in fp64.  Order of a row's sum: thread t adds its columns j = t, t + 256, ... in that order from +0.0;
// v += shfl_down(v, o) for o = 32, 16, 8, 4, 2, 1 within a wave; ((wave 0 + wave 1) + wave 2) + wave 3.
template <int KL> __global__ __launch_bounds__(TS_PT) void tsne_pass_kernel(const float* __restrict__ p, const float* __restrict__ y, int n,
                                                                             double* __restrict__ rows) {
  constexpr int NA = KL ? 3 : 5;
  __shared__ double part[TS_PT / 64][TS_R][NA];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i0 = blockIdx.x * TS_R;
  float yi0[TS_R], yi1[TS_R];
  const float* prow[TS_R];
  double acc[TS_R][NA];
#pragma unroll
  for (int r = 0; r < TS_R; ++r) {
    const int i = min(i0 + r, n - 1);                                    // a row past the table reads the last one; its sums are not stored
    yi0[r] = y[2 * i]; yi1[r] = y[2 * i + 1];
    prow[r] = p + (size_t)i * n;
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[r][a] = 0.0;
  }
  const float2* y2 = reinterpret_cast<const float2*>(y);
  float2 ynext = make_float2(0.f, 0.f);
  float pnext[TS_R];
  if (tid < n) {
    ynext = y2[tid];
#pragma unroll
    for (int r = 0; r < TS_R; ++r) pnext[r] = prow[r][tid];
  }
  for (int j = tid; j < n; j += TS_PT) {
    const float2 yj = ynext;
    float pv[TS_R];
#pragma unroll
    for (int r = 0; r < TS_R; ++r) pv[r] = pnext[r];
    if (j + TS_PT < n) {                                                 // the next step's loads are in flight while this one is computed
      ynext = y2[j + TS_PT];
#pragma unroll
      for (int r = 0; r < TS_R; ++r) pnext[r] = prow[r][j + TS_PT];
    }
#pragma unroll
    for (int r = 0; r < TS_R; ++r) {
      const float dx = yi0[r] - yj.x, dy = yi1[r] - yj.y;
      const float d2 = dx * dx + dy * dy;
      const float w = 1.0f / (1.0f + d2);
      const double wd = (double)w, self = (j == i0 + r) ? 0.0 : wd;
      if (KL) {
        if (pv[r] > 0.f) acc[r][0] = acc[r][0] + (double)pv[r] * (log((double)pv[r]) - log(wd));
        acc[r][1] = acc[r][1] + (double)pv[r];
        acc[r][2] = acc[r][2] + self;
      } else {
        const double pw = (double)pv[r] * wd, ww = wd * wd;
        acc[r][0] = acc[r][0] + pw * (double)dx;
        acc[r][1] = acc[r][1] + pw * (double)dy;
        acc[r][2] = acc[r][2] + ww * (double)dx;
        acc[r][3] = acc[r][3] + ww * (double)dy;
        acc[r][4] = acc[r][4] + self;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < TS_R; ++r)
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      double v = acc[r][a];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o);
      if (lane == 0) part[wv][r][a] = v;
    }
  __syncthreads();
  if (tid < TS_R * NA) {
    const int r = tid / NA, a = tid - r * NA;
    const double v = ((part[0][r][a] + part[1][r][a]) + part[2][r][a]) + part[3][r][a];
    if (i0 + r < n) rows[(size_t)(i0 + r) * NA + a] = v;
  }
}

// column `col` of rows [n][stride], every thread gets it: thread t adds the rows t, t + 256, ... in that order from +0.0, then block_tree_sum
__device__ __forceinline__ double tsne_column_sum(const double* __restrict__ rows, int n, int stride, int col, double* red, int tid) {
  double s[1] = {0.0};
  for (int i = tid; i < n; i += 256) s[0] = s[0] + rows[(size_t)i * stride + col];
  block_tree_sum<256, 1>(s, red, tid);
  return s[0];
}

// g_ic = (float)(4 (e A_ic - B_ic / Z)), fp64
__global__ __launch_bounds__(256) void tsne_combine_kernel(const double* __restrict__ rows, int n, double ex, float* __restrict__ grad,
                                                            double* __restrict__ z_out) {
  __shared__ double red[256];
  const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
  const double z = tsne_column_sum(rows, n, 5, 4, red, tid);
  if (i < n) {
    const double* r = rows + (size_t)i * 5;
    grad[2 * i] = (float)(4.0 * (ex * r[0] - r[2] / z));
    grad[2 * i + 1] = (float)(4.0 * (ex * r[1] - r[3] / z));
  }
  if (blockIdx.x == 0 && tid == 0 && z_out) *z_out = z;
}

// kl = sum_i K_i + log(Z) sum_i P_i
__global__ __launch_bounds__(256) void tsne_kl_join_kernel(const double* __restrict__ rows, int n, double* __restrict__ kl) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const double k = tsne_column_sum(rows, n, 3, 0, red, tid);
  const double ps = tsne_column_sum(rows, n, 3, 1, red, tid);
  const double z = tsne_column_sum(rows, n, 3, 2, red, tid);
  if (tid == 0) *kl = k + log(z) * ps;
}

__device__ __forceinline__ int tsne_sign(float v) { return v > 0.f ? 1 : v < 0.f ? -1 : 0; }      // +-0 (and NaN): 0

__global__ __launch_bounds__(2 * ROWS_PER_BLOCK) void tsne_update_kernel(float* __restrict__ y, const float* __restrict__ grad, float* __restrict__ inc,
                                                                  float* __restrict__ gains, int n, float eta, float momentum, float min_gain,
                                                                  double* __restrict__ part /*[blocks][2]*/) {
  __shared__ double ys[2 * ROWS_PER_BLOCK];
  const int tid = threadIdx.x;
  const long e = (long)blockIdx.x * 2 * ROWS_PER_BLOCK + tid;
  double v = 0.0;
  if (e < 2L * n) {
    const float g = grad[e], u = inc[e];
    float ga = gains[e];
    ga = tsne_sign(g) == tsne_sign(u) ? ga * 0.8f : ga + 0.2f;
    if (ga < min_gain) ga = min_gain;
    const float step = (eta * ga) * g;
    const float nu = momentum * u - step;
    const float ny = y[e] + nu;
    gains[e] = ga; inc[e] = nu; y[e] = ny;
    v = (double)ny;
  }
  ys[tid] = v;
  __syncthreads();
  if (tid < 2) {                                                         // the block's rows in row order (rows past the table add +0.0: no change)
    double s = 0.0;
#pragma unroll 8
    for (int r = 0; r < ROWS_PER_BLOCK; ++r) s = s + ys[2 * r + tid];
    part[2 * blockIdx.x + tid] = s;
  }
}

__global__ __launch_bounds__(256) void tsne_centre_kernel(float* __restrict__ y, int n, const double* __restrict__ part, int nblk) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2L * n) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s = s + part[2 * b + (int)(e & 1)];
  y[e] = (float)((double)y[e] - s / (double)n);
}

// ------------------------------------------------------------------ gr_map_cells_dev
__global__ __launch_bounds__(1024) void cells_box_kernel(const float* __restrict__ y, long n, float* __restrict__ box /*lo0, lo1, hi0, hi1*/) {
  __shared__ float red[4][1024];
  const int tid = threadIdx.x;
  float lo0 = INFINITY, lo1 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY;
  for (long i = tid; i < n; i += 1024) {
    const float a = y[2 * i], b = y[2 * i + 1];
    lo0 = a < lo0 ? a : lo0; hi0 = a > hi0 ? a : hi0;
    lo1 = b < lo1 ? b : lo1; hi1 = b > hi1 ? b : hi1;
  }
  red[0][tid] = lo0; red[1][tid] = lo1; red[2][tid] = hi0; red[3][tid] = hi1;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] = red[0][tid + o] < red[0][tid] ? red[0][tid + o] : red[0][tid];
      red[1][tid] = red[1][tid + o] < red[1][tid] ? red[1][tid + o] : red[1][tid];
      red[2][tid] = red[2][tid + o] > red[2][tid] ? red[2][tid + o] : red[2][tid];
      red[3][tid] = red[3][tid + o] > red[3][tid] ? red[3][tid + o] : red[3][tid];
    }
    __syncthreads();
  }
  if (tid < 4) box[tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void cells_clear_kernel(unsigned long long* __restrict__ keys, int* __restrict__ counts, int cells) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  keys[c] = ~0ULL;
  if (counts) counts[c] = 0;
}

// the cell of v on an axis [lo, hi] cut in g: min(g - 1, (int)(((v - lo) / (hi - lo)) * (float)g)), 0 on a degenerate axis
__device__ __forceinline__ int cells_axis(float v, float lo, float hi, int g) {
  if (!(hi > lo)) return 0;
  const float t = ((v - lo) / (hi - lo)) * (float)g;
  const int c = (int)t;
  return c < g - 1 ? (c < 0 ? 0 : c) : g - 1;
}
// the centre of cell c: lo + ((float)c + 0.5f) * ((hi - lo) / (float)g)
__device__ __forceinline__ float cells_centre(int c, float lo, float hi, int g) { return lo + ((float)c + 0.5f) * ((hi - lo) / (float)g); }

__global__ __launch_bounds__(256) void cells_assign_kernel(const float* __restrict__ y, long n, int gh, int gw, const float* __restrict__ box,
                                                            unsigned long long* __restrict__ keys, int* __restrict__ counts) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float a = y[2 * i], b = y[2 * i + 1];
  const int cx = cells_axis(a, box[0], box[2], gw), cy = cells_axis(b, box[1], box[3], gh);
  const float da = a - cells_centre(cx, box[0], box[2], gw), db = b - cells_centre(cy, box[1], box[3], gh);
  const float d2 = da * da + db * db;                                    // >= 0: its bit pattern orders like the number
  const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(unsigned)i;
  const int cell = cy * gw + cx;
  atomicMin(&keys[cell], key);                                           // a 64-bit integer minimum: (distance, row), ties to the lower row
  if (counts) atomicAdd(&counts[cell], 1);
}

__global__ __launch_bounds__(256) void cells_unpack_kernel(const unsigned long long* __restrict__ keys, int cells, long* __restrict__ rows_out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const unsigned long long k = keys[c];
  rows_out[c] = k == ~0ULL ? -1L : (long)(k & 0xFFFFFFFFULL);
}

// ------------------------------------------------------------------ launchers
size_t tsne_affinities_workspace_bytes(int n, int d) { return sizeof(float) * (size_t)n * d + 256; }
size_t tsne_iter_workspace_bytes(int n) { return sizeof(double) * ((size_t)n * 5 + 2 * (size_t)row_blocks(n)) + 512; }
size_t map_cells_workspace_bytes(int cells) { return 8 * (size_t)cells + 256; }

int launch_tsne_affinities(const float* x, int n, int d, double perplexity, float* p, double* beta, int* info, void* workspace, hipStream_t s) {
  if (n < 4 || n > TS_MAX_N || d < 1) return 1;
  float* xt = reinterpret_cast<float*>(workspace);
  if (hipMemsetAsync(info, 0, 2 * sizeof(int), s) != hipSuccess) return 2;
  { KtScope kt("tsne_cond_kernel", 3.0 * n * n * d, 4.0 * n * n * d, s);
    hipLaunchKernelGGL(tsne_transpose_kernel, dim3((unsigned)(((size_t)n * d + 255) / 256)), dim3(256), 0, s, x, n, d, xt);
    hipLaunchKernelGGL(tsne_cond_kernel, dim3(n), dim3(TS_CT), 0, s, x, xt, n, d, log(perplexity), p, beta, info); }
  const int nt = (n + 31) / 32;
  KtScope kt("tsne_symm_kernel", 0.0, 8.0 * n * n, s);
  hipLaunchKernelGGL(tsne_symm_kernel, dim3(nt, nt), dim3(256), 0, s, p, n);
  return 0;
}

int launch_tsne_gradient(const float* p, const float* y, int n, float exaggeration, float* grad, double* z, void* workspace, hipStream_t s) {
  if (n < 1 || n > TS_MAX_N) return 1;
  double* rows = reinterpret_cast<double*>(workspace);
  { KtScope kt("tsne_pass_kernel", 27.0 * n * n, 4.0 * n * n, s);
    hipLaunchKernelGGL(tsne_pass_kernel<0>, dim3((n + TS_R - 1) / TS_R), dim3(TS_PT), 0, s, p, y, n, rows); }
  KtScope kt("tsne_combine_kernel", 0.0, 40.0 * n, s);
  hipLaunchKernelGGL(tsne_combine_kernel, dim3((n + 255) / 256), dim3(256), 0, s, rows, n, (double)exaggeration, grad, z);
  return 0;
}

int launch_tsne_kl(const float* p, const float* y, int n, double* kl, void* workspace, hipStream_t s) {
  if (n < 1 || n > TS_MAX_N) return 1;
  double* rows = reinterpret_cast<double*>(workspace);
  KtScope kt("tsne_kl_kernel", 0.0, 4.0 * n * n, s);
  hipLaunchKernelGGL(tsne_pass_kernel<1>, dim3((n + TS_R - 1) / TS_R), dim3(TS_PT), 0, s, p, y, n, rows);
  hipLaunchKernelGGL(tsne_kl_join_kernel, dim3(1), dim3(256), 0, s, rows, n, kl);
  return 0;
}

int launch_tsne_update(float* y, const float* grad, float* inc, float* gains, int n, float eta, float momentum, float min_gain, void* workspace,
                       hipStream_t s) {
  if (n < 1 || n > TS_MAX_N) return 1;
  double* part = reinterpret_cast<double*>(workspace) + (size_t)n * 5;      // behind the gradient's row sums: one workspace serves an iteration
  const int nblk = (int)row_blocks(n);
  KtScope kt("tsne_update_kernel", 0.0, 40.0 * n, s);
  hipLaunchKernelGGL(tsne_update_kernel, dim3(nblk), dim3(2 * ROWS_PER_BLOCK), 0, s, y, grad, inc, gains, n, eta, momentum, min_gain, part);
  hipLaunchKernelGGL(tsne_centre_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, s, y, n, part, nblk);
  return 0;
}

int launch_map_cells(const float* y, long n, int gh, int gw, long* rows_out, int* counts, void* workspace, hipStream_t s) {
  if (n < 1 || n > 0x7FFFFFFFL || gh < 1 || gw < 1 || gh > 1024 || gw > 1024) return 1;
  const int cells = gh * gw;
  float* box = reinterpret_cast<float*>(workspace);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(workspace) + 256);
  KtScope kt("map_cells_kernel", 0.0, 16.0 * n, s);
  hipLaunchKernelGGL(cells_box_kernel, dim3(1), dim3(1024), 0, s, y, n, box);
  hipLaunchKernelGGL(cells_clear_kernel, dim3((cells + 255) / 256), dim3(256), 0, s, keys, counts, cells);
  hipLaunchKernelGGL(cells_assign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, n, gh, gw, box, keys, counts);
  hipLaunchKernelGGL(cells_unpack_kernel, dim3((cells + 255) / 256), dim3(256), 0, s, keys, cells, rows_out);
  return 0;
}

}  // namespace gr
