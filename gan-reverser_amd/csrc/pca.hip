// pca.hip — principal axes of a device table [n x d], d <= 256 (gr_pca_dev, gr_pca_project_dev; new: no counterpart in the reference).
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/pca_paths.py; this file is compiled without FMA contraction
// (Makefile), so every fp32 multiply and add below rounds on its own.  No floating-point atomics, no grid barrier: every result is a function
// of the inputs alone.
//
// Kernels:
//   pca_mean_kernel       workgroup = max(1, 256 / d) blocks of 512 consecutive rows, thread = (block, column): the block's rows added in row
//                         order in fp64 -> one partial per block
//   pca_mean_join_kernel  thread = column: the block partials in block order from +0.0 (ordered_sum8, kernels.h), one division by n
//   pca_cov_kernel        workgroup = (64 x 64 tile of C with tile row <= tile column, one of PCA_P contiguous ranges of 512-row blocks); the
//                         centred rows c = (float)((double)x - mean) go through LDS 64 at a time; thread = 4 x 4 elements, each one sequential
//                         fp32 chain over the block's rows (acc = acc + c_i * c_j), added to the thread's fp64 sums when the block ends
//   pca_cov_join_kernel   element (i <= j): the PCA_P partials in order from +0.0, one division by n - 1, written to [i][j] and [j][i]
//   pca_jacobi_kernel     ONE workgroup of 1024 threads: cyclic Jacobi in fp64 with the round-robin ordering - floor(d / 2) disjoint rotations
//                         between two workgroup barriers; A and V^T live in context scratch (512 KB each at d = 256: L2)
//   pca_project_kernel    workgroup = 128 centred rows held in LDS (stage_rows, kernels.h), axis tiles of 128 staged 32 columns at a time (kmeans_assign_wide_kernel's
//                         shape): thread = 4 rows x 16 axes, every (row, axis) one sequential fp32 chain in column order
#include "kernels.h"

namespace gr {

constexpr int PCA_P = 128;              // partial covariance matrices: a constant of the library (tests/pca_paths.py restates it)
constexpr int PCA_T = 64, PCA_KC = 64;  // tile of C per workgroup; rows per LDS stage
constexpr int PCA_DMAX = 256;
constexpr int PCA_JT = 1024;            // threads of the Jacobi workgroup
constexpr int PCA_JB = 4, PCA_VB = 8;   // 2 x 2 blocks of A / row-pair elements of V^T a thread has in flight
constexpr int PCA_SWEEP_CAP = 30;       // sweeps at most (info[1] = 0 when they run out)
constexpr double PCA_TAU2 = 0x1p-92;    // tau^2, tau = 2^-46: stop when off(A)_F^2 <= tau^2 ||A||_F^2

__global__ __launch_bounds__(256) void pca_mean_kernel(const float* __restrict__ x, long n, long nblk, int d, double* __restrict__ part /*[nblk][d]*/) {
  const int per = max(1, 256 / d), sub = threadIdx.x / d, t = threadIdx.x - sub * d;      // a workgroup takes as many blocks as its threads hold columns
  const long blk = (long)blockIdx.x * per + sub;
  if (sub >= per || blk >= nblk) return;
  const long r0 = blk * ROWS_PER_BLOCK;
  const int nr = (int)min((long)ROWS_PER_BLOCK, n - r0);
  const float* src = x + r0 * d + t;
  double s = 0.0;
  for (int r = 0; r < nr; r += 8) {                    // eight loads in flight, then the adds in row order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = r + u < nr ? src[(long)(r + u) * d] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r + u < nr) s += (double)v[u];
  }
  part[blk * d + t] = s;
}

__global__ __launch_bounds__(256) void pca_mean_join_kernel(const double* __restrict__ part, long nblk, long n, int d, double* __restrict__ mean) {
  const int t = threadIdx.x;
  if (t >= d) return;
  mean[t] = ordered_sum8(part + t, nblk, d) / (double)n;
}

__global__ __launch_bounds__(256) void pca_cov_kernel(const float* __restrict__ x, long n, int d, const double* __restrict__ mean, int ntile,
                                                       double* __restrict__ part /*[PCA_P][d][d], tiles with ti <= tj*/) {
  __shared__ __attribute__((aligned(16))) float As[PCA_KC][PCA_T];
  __shared__ __attribute__((aligned(16))) float Bs[PCA_KC][PCA_T];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, p = blockIdx.y;
  int ti = 0, rem = blockIdx.x;
  while (rem >= ntile - ti) { rem -= ntile - ti; ++ti; }
  const int tj = ti + rem;
  const long nblk = row_blocks(n);
  const long b_lo = p * nblk / PCA_P, b_hi = (p + 1) * nblk / PCA_P;      // contiguous, uneven ranges; empty ones when nblk < PCA_P
  const int c = tid & 63, rs = tid >> 6;                                   // this thread stages column c of rows rs, rs + 4, ...
  const int ca = ti * PCA_T + c, cb = tj * PCA_T + c;
  const double ma = ca < d ? mean[ca] : 0.0, mb = cb < d ? mean[cb] : 0.0;
  const float (*Bp)[PCA_T] = ti == tj ? As : Bs;
  double sum[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) sum[a][b] = 0.0;
  // The range's rows in stages of PCA_KC; a block is ROWS_PER_BLOCK / PCA_KC stages (only the table's last block may have fewer).  The raw values of
  // stage s + 1 are fetched into registers while stage s is multiplied.
  const long row_lo = b_lo * ROWS_PER_BLOCK, row_hi = min(b_hi * ROWS_PER_BLOCK, n);
  const long nstage = row_hi > row_lo ? (row_hi - row_lo + PCA_KC - 1) / PCA_KC : 0;
  constexpr int SPB = ROWS_PER_BLOCK / PCA_KC, NU = PCA_KC / 4;
  float va[NU], vb[NU], acc[4][4];
  auto fetch = [&](long s) {
    const long base = row_lo + s * PCA_KC + rs;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const long r = base + 4 * u;
      const bool in = r < row_hi;
      va[u] = (in && ca < d) ? x[r * d + ca] : 0.f;
      vb[u] = (in && cb < d && ti != tj) ? x[r * d + cb] : 0.f;
    }
  };
  if (nstage) fetch(0);
  for (long s = 0; s < nstage; ++s) {
    const long base = row_lo + s * PCA_KC + rs;
    __syncthreads();                                                       // the stage before this one has been read
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int r = rs + 4 * u;
      const bool in = base + 4 * u < row_hi;
      As[r][c] = (in && ca < d) ? (float)((double)va[u] - ma) : 0.f;       // rows past the range and columns past d: +0, which changes no sum
      if (ti != tj) Bs[r][c] = (in && cb < d) ? (float)((double)vb[u] - mb) : 0.f;
    }
    __syncthreads();
    if (s + 1 < nstage) fetch(s + 1);
    if (s % SPB == 0) {                                                    // a block begins: its chains start from +0
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    }
#pragma unroll 8
    for (int r = 0; r < PCA_KC; ++r) {
      const float4 av = *reinterpret_cast<const float4*>(&As[r][ty * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&Bp[r][tx * 4]);
      const float a4[4] = {av.x, av.y, av.z, av.w}, b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = acc[a][b] + a4[a] * b4[b];             // no contraction (Makefile): rounded multiply, rounded add
    }
    if (s % SPB == SPB - 1 || s + 1 == nstage) {                           // the block ends: fp64 joins the blocks, in block order
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) sum[a][b] += (double)acc[a][b];
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = ti * PCA_T + ty * 4 + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = tj * PCA_T + tx * 4 + b;
      if (i < d && j < d) part[((long)p * d + i) * d + j] = sum[a][b];
    }
  }
}

// C[i][j] (i <= j) = (the partials in order from +0.0) / (n - 1) -> a [d][d] (the Jacobi's working copy) and cov (nullable), both triangles
__global__ __launch_bounds__(256) void pca_cov_join_kernel(const double* __restrict__ part, long n, int d, double* __restrict__ a, double* __restrict__ cov) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e - i * d;
  if (i > j) return;
  double s = 0.0;
  for (int p = 0; p < PCA_P; ++p) s += part[((long)p * d + i) * d + j];
  const double v = s / (double)(n - 1);
  a[i * d + j] = v; a[j * d + i] = v;
  if (cov) { cov[i * d + j] = v; cov[j * d + i] = v; }
}

// block_tree_sum of one value per thread, out of line: the Jacobi kernel calls it twice and keeps its registers for the rotations
__device__ __noinline__ double pca_block_sum(double v, double* red, int tid) {
  double a[1] = {v};
  block_tree_sum<PCA_JT, 1>(a, red, tid);
  return a[0];
}

// a [d][d] symmetric in (both triangles the same bits; destroyed), vt [d][d] scratch (row = eigenvector).  Round r of a sweep pairs the m = d + (d & 1)
// players by the circle method: pair 0 = (m - 1, r), pair k = ((r + k) mod (m - 1), (r - k) mod (m - 1)); a pair with player d (odd d) has a bye.
// Per round: every pair's rotation from its 2 x 2 pivot block (skipped when the off-diagonal element is exactly 0), a barrier, then
// A <- J^T A J one 2 x 2 block per (pair, pair) - the rotation of the pair with the lower index first, in both triangles, so that A stays
// symmetric bit for bit - and V^T <- J^T V^T row pair by row pair, a barrier.
__global__ __launch_bounds__(PCA_JT) void pca_jacobi_kernel(double* a, double* vt, int d, double* __restrict__ eigvals, float* __restrict__ axes,
                                                             int* __restrict__ info) {
  __shared__ double red[PCA_JT];
  __shared__ double cc[PCA_DMAX / 2], ss[PCA_DMAX / 2], tt[PCA_DMAX / 2], lam[PCA_DMAX];
  __shared__ int pp[PCA_DMAX / 2], qq[PCA_DMAX / 2], rk[PCA_DMAX];
  __shared__ float sg[PCA_DMAX];
  const int tid = threadIdx.x, dd = d * d;
  double s = 0.0;
  for (int e = tid; e < dd; e += PCA_JT) {
    const int i = e / d, j = e - i * d;
    vt[e] = i == j ? 1.0 : 0.0;
    s += a[e] * a[e];
  }
  const double norm2 = pca_block_sum(s, red, tid);
  const int m = d + (d & 1), np = m / 2;
  int sweeps = 0, converged = 0;
  for (;;) {
    s = 0.0;
    for (int e = tid; e < dd; e += PCA_JT) {
      const int i = e / d, j = e - i * d;
      if (i != j) s += a[e] * a[e];
    }
    const double off2 = pca_block_sum(s, red, tid);
    if (off2 <= PCA_TAU2 * norm2) { converged = 1; break; }
    if (sweeps == PCA_SWEEP_CAP) break;
    for (int r = 0; r < m - 1; ++r) {
      if (tid < np) {
        const int u = tid == 0 ? m - 1 : (r + tid) % (m - 1), v = tid == 0 ? r : (r - tid + (m - 1)) % (m - 1);
        const int p = u < d ? u : v, q = u < d ? v : d;                    // the pair as listed: consecutive pairs have consecutive columns
        double c = 1.0, sn = 0.0, t = 0.0;
        if (q < d) {
          const double apq = a[p * d + q];
          if (apq != 0.0) {                                               // an element that is exactly 0 needs no rotation (and would give 0 / 0)
            const double tau = (a[q * d + q] - a[p * d + p]) / (2.0 * apq);
            t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            sn = t * c;
          }
        }
        pp[tid] = p; qq[tid] = q < d ? q : -1;                            // the bye: p alone, with the identity (c = 1, s = 0) - its row and
        cc[tid] = c; ss[tid] = sn; tt[tid] = t;                           // column still take the other pairs' rotations
      }
      __syncthreads();
      // Every block (ki, kj) has its own thread, which reads and writes nothing else: PCA_JB blocks at a time, all loads, then the arithmetic, then
      // all stores.  kj runs fastest, and consecutive pairs hold consecutive columns: every access is along a row of A.  Blocks (ki, kj) and
      // (kj, ki) apply the two rotations in the same order - the pair with the lower index first - to transposed operands, so their results are
      // transposes of each other bit for bit and A stays symmetric without anybody writing the other triangle.
      for (int e0 = tid; e0 < np * np; e0 += PCA_JT * PCA_JB) {
        int ki[PCA_JB], kj[PCA_JB];
        bool on[PCA_JB];
        double x11[PCA_JB], x12[PCA_JB], x21[PCA_JB], x22[PCA_JB];
#pragma unroll
        for (int u = 0; u < PCA_JB; ++u) {
          const int e = e0 + u * PCA_JT;
          ki[u] = e / np; kj[u] = e - ki[u] * np;
          on[u] = e < np * np;
          x11[u] = x12[u] = x21[u] = x22[u] = 0.0;
          if (on[u]) {
            const int pi = pp[ki[u]], qi = qq[ki[u]], pj = pp[kj[u]], qj = qq[kj[u]];
            if (ki[u] == kj[u] && qi < 0) on[u] = false;                  // the bye's own diagonal element stays
            else {                                                        // (q < 0: the bye's single row / column; its absent partner reads as 0)
              x11[u] = a[pi * d + pj];
              if (qj >= 0) x12[u] = a[pi * d + qj];
              if (qi >= 0) x21[u] = a[qi * d + pj];
              if (qi >= 0 && qj >= 0) x22[u] = a[qi * d + qj];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < PCA_JB; ++u) {
          if (!on[u]) continue;
          const int pi = pp[ki[u]], qi = qq[ki[u]], pj = pp[kj[u]], qj = qq[kj[u]];
          if (ki[u] == kj[u]) {                                           // the pivot block in closed form: a_pp - t a_pq, a_qq + t a_pq, 0
            const double apq = x12[u], t = tt[ki[u]];
            a[pi * d + pi] = x11[u] - t * apq;
            a[qi * d + qi] = x22[u] + t * apq;
            if (apq != 0.0) { a[pi * d + qi] = 0.0; a[qi * d + pi] = 0.0; }
            continue;
          }
          const double ci = cc[ki[u]], si = ss[ki[u]], cj = cc[kj[u]], sj = ss[kj[u]];
          double n11, n12, n21, n22;
          if (ki[u] < kj[u]) {                                            // J_i^T from the left, then J_j from the right
            const double b11 = ci * x11[u] - si * x21[u], b21 = si * x11[u] + ci * x21[u];
            const double b12 = ci * x12[u] - si * x22[u], b22 = si * x12[u] + ci * x22[u];
            n11 = cj * b11 - sj * b12; n12 = sj * b11 + cj * b12;
            n21 = cj * b21 - sj * b22; n22 = sj * b21 + cj * b22;
          } else {                                                        // J_j from the right, then J_i^T from the left
            const double b11 = cj * x11[u] - sj * x12[u], b12 = sj * x11[u] + cj * x12[u];
            const double b21 = cj * x21[u] - sj * x22[u], b22 = sj * x21[u] + cj * x22[u];
            n11 = ci * b11 - si * b21; n21 = si * b11 + ci * b21;
            n12 = ci * b12 - si * b22; n22 = si * b12 + ci * b22;
          }
          a[pi * d + pj] = n11;
          if (qj >= 0) a[pi * d + qj] = n12;
          if (qi >= 0) a[qi * d + pj] = n21;
          if (qi >= 0 && qj >= 0) a[qi * d + qj] = n22;
        }
      }
      for (int e0 = tid; e0 < np * d; e0 += PCA_JT * PCA_VB) {                // the row pairs of V^T the same way
        int ip[PCA_VB], iq[PCA_VB], kk[PCA_VB];
        double vp[PCA_VB], vq[PCA_VB];
#pragma unroll
        for (int u = 0; u < PCA_VB; ++u) {
          const int e = e0 + u * PCA_JT, k = e / d, j = e - k * d;
          kk[u] = e < np * d && qq[min(k, np - 1)] >= 0 ? k : -1;
          if (kk[u] >= 0) { ip[u] = pp[k] * d + j; iq[u] = qq[k] * d + j; vp[u] = vt[ip[u]]; vq[u] = vt[iq[u]]; }
        }
#pragma unroll
        for (int u = 0; u < PCA_VB; ++u)
          if (kk[u] >= 0) {
            const double c = cc[kk[u]], sn = ss[kk[u]];
            vt[ip[u]] = c * vp[u] - sn * vq[u];
            vt[iq[u]] = sn * vp[u] + c * vq[u];
          }
      }
      __syncthreads();
    }
    ++sweeps;
  }
  // eigenvalues descending, ties by ascending column (a NaN after every number); each axis signed so that its first largest component is positive
  if (tid < d) lam[tid] = a[tid * d + tid];
  __syncthreads();
  if (tid < d) {
    const double l = lam[tid];
    const bool ln = l != l;
    int rank = 0;
    for (int b = 0; b < d; ++b) {
      const double o = lam[b];
      const bool on = o != o;
      const bool before = ln ? (!on || b < tid) : (!on && (o > l || (o == l && b < tid)));
      rank += before ? 1 : 0;
    }
    rk[tid] = rank;
    eigvals[rank] = l;
    float best = 0.f, sign = 1.f;
    for (int t = 0; t < d; ++t) {
      const float v = (float)vt[tid * d + t];
      if (fabsf(v) > best) { best = fabsf(v); sign = v < 0.f ? -1.f : 1.f; }
    }
    sg[tid] = sign;
  }
  __syncthreads();
  for (int e = tid; e < dd; e += PCA_JT) {
    const int i = e / d, t = e - i * d;
    axes[rk[i] * d + t] = sg[i] * (float)vt[e];
  }
  if (tid == 0) { info[0] = sweeps; info[1] = converged; }
}

// ------------------------------------------------------------------ projection
constexpr int PJ_TR = 128, PJ_RT = 4, PJ_AT = 128, PJ_DC = 32, PJ_CLD = 132;   // rows: 32 lanes x PJ_RT; axes of a tile: 4 waves x 2 half-waves x 16

__global__ __launch_bounds__(256) void pca_project_kernel(const float* __restrict__ x, long n, int d, const double* __restrict__ mean,
                                                           const float* __restrict__ axes, const double* __restrict__ eigvals, int k, int whiten,
                                                           float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float xs[];            // [PJ_TR][ld], ld odd: the centred rows
  __shared__ __attribute__((aligned(16))) float cs[PJ_DC * PJ_CLD];     // [column of the chunk][axis of the tile]
  __shared__ double ms[PCA_DMAX];
  const int tid = threadIdx.x, w = tid >> 6, rl = tid & 31, hw = tid >> 5;
  const int ld = d | 1;
  const long r0 = (long)blockIdx.x * PJ_TR;
  const int nr = (int)min((long)PJ_TR, n - r0);
  if (tid < d) ms[tid] = mean[tid];
  __syncthreads();
  stage_rows<PJ_TR>(x, r0, nr, d, ld, xs, tid, [&](float v, int c) { return (float)((double)v - ms[c]); });      // centred on the way in
  for (int j0 = 0; j0 < k; j0 += PJ_AT) {
    float acc[PJ_RT][16];
#pragma unroll
    for (int q = 0; q < PJ_RT; ++q)
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) acc[q][jj] = 0.f;
    for (int c0 = 0; c0 < d; c0 += PJ_DC) {
      const int dc = min(PJ_DC, d - c0);
      __syncthreads();                                                  // the chunk before this one has been read (and xs is written)
      for (int e = tid; e < PJ_DC * PJ_AT; e += 256) {
        const int jj = e / PJ_DC, cc = e - jj * PJ_DC;
        cs[cc * PJ_CLD + jj] = (j0 + jj < k && cc < dc) ? axes[(long)(j0 + jj) * d + c0 + cc] : 0.f;
      }
      __syncthreads();
      if (j0 + w * 32 < k)                                              // (wave-uniform; a half-wave past k multiplies the tile's zero padding)
        for (int c = 0; c < dc; ++c) {
          float xv[PJ_RT];
#pragma unroll
          for (int q = 0; q < PJ_RT; ++q) xv[q] = xs[(rl + 32 * q) * ld + c0 + c];
          const float4* cp = reinterpret_cast<const float4*>(cs + c * PJ_CLD + hw * 16);
          float cv[16];
#pragma unroll
          for (int g = 0; g < 4; ++g) { const float4 v = cp[g]; cv[4 * g] = v.x; cv[4 * g + 1] = v.y; cv[4 * g + 2] = v.z; cv[4 * g + 3] = v.w; }
#pragma unroll
          for (int q = 0; q < PJ_RT; ++q)
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) acc[q][jj] = acc[q][jj] + xv[q] * cv[jj];      // no contraction (Makefile): one chain per (row, axis)
        }
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = j0 + hw * 16 + jj;
      if (j < k) {
        double scale = 1.0;
        bool zero = false;
        if (whiten) { const double ev = eigvals[j]; zero = !(ev > 0.0); scale = zero ? 0.0 : 1.0 / sqrt(ev); }
#pragma unroll
        for (int q = 0; q < PJ_RT; ++q) {
          const int r = rl + 32 * q;
          if (r < nr) out[(r0 + r) * k + j] = !whiten ? acc[q][jj] : zero ? 0.f : (float)((double)acc[q][jj] * scale);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ launchers
// block partials of the mean [ceil(n / 512)][d], the PCA_P partial matrices, A and V^T: all doubles
size_t pca_workspace_bytes(long n, int d) {
  const size_t nblk = (size_t)row_blocks(n);
  return sizeof(double) * (nblk * d + (size_t)PCA_P * d * d + 2 * (size_t)d * d) + 1024;
}

int launch_pca(const float* x, long n, int d, double* mean, double* cov, double* eigvals, float* axes, int* info, void* workspace, hipStream_t s) {
  if (n < 2 || n > 0x7FFFFFFFL || d < 1 || d > PCA_DMAX) return 1;
  const long nblk = row_blocks(n);
  double* part_mean = reinterpret_cast<double*>(workspace);
  double* part_cov = part_mean + (size_t)nblk * d;
  double* a = part_cov + (size_t)PCA_P * d * d;
  double* vt = a + (size_t)d * d;
  { KtScope kt("pca_mean_kernel", (double)n * d, 4.0 * n * d, s);
    const int per = 256 / d > 1 ? 256 / d : 1;
    hipLaunchKernelGGL(pca_mean_kernel, dim3((unsigned)((nblk + per - 1) / per)), dim3(256), 0, s, x, n, nblk, d, part_mean);
    hipLaunchKernelGGL(pca_mean_join_kernel, dim3(1), dim3(256), 0, s, part_mean, nblk, n, d, mean); }
  const int ntile = (d + PCA_T - 1) / PCA_T;
  { KtScope kt("pca_cov_kernel", (double)n * d * (d + 1), 4.0 * n * d, s);
    hipLaunchKernelGGL(pca_cov_kernel, dim3(ntile * (ntile + 1) / 2, PCA_P), dim3(256), 0, s, x, n, d, mean, ntile, part_cov);
    hipLaunchKernelGGL(pca_cov_join_kernel, dim3((d * d + 255) / 256), dim3(256), 0, s, part_cov, n, d, a, cov); }
  KtScope kt("pca_jacobi_kernel", 0.0, 16.0 * d * d, s);
  hipLaunchKernelGGL(pca_jacobi_kernel, dim3(1), dim3(PCA_JT), 0, s, a, vt, d, eigvals, axes, info);
  return 0;
}

// returns 1 outside 1 <= n < 2^31, 1 <= k <= d <= 256, and 2 when the device refuses the kernel's LDS
int launch_pca_project(const float* x, long n, int d, const double* mean, const float* axes, const double* eigvals, int k, int whiten, float* out,
                       hipStream_t s) {
  if (n < 1 || n > 0x7FFFFFFFL || d < 1 || d > PCA_DMAX || k < 1 || k > d) return 1;
  const size_t lds = sizeof(float) * PJ_TR * (size_t)(d | 1);
  if (lds > 32 * 1024)                                                   // (per device; a host-side setting, cheap to repeat)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(pca_project_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(sizeof(float) * PJ_TR * 257)) != hipSuccess) return 2;
  KtScope kt("pca_project_kernel", 2.0 * n * d * k, 4.0 * n * (d + k), s);
  hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)((n + PJ_TR - 1) / PJ_TR)), dim3(256), lds, s, x, n, d, mean, axes, eigvals, k, whiten, out);
  return 0;
}

}  // namespace gr
