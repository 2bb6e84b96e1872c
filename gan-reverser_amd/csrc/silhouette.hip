// silhouette.hip — silhouette coefficients of a labelled device table [n x d], n <= 262144, d <= 256, k <= 4096 (gr_silhouette_dev; new: no
// counterpart in the reference, whose README asks whether "other clustering methods would produce better results" - this is the score that says).
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/silhouette_paths.py; this file is compiled without FMA contraction
// (Makefile), so every multiply and add below rounds on its own.  Everything past the loads is fp64: x enters by an exact conversion.  No
// floating-point atomics, no grid barrier: every result is a function of the inputs alone.
//
// Operation by operation (all fp64, sqrt the device library's correctly rounded one):
//   pair distance, euclidean   t = x_it - x_jt;  D = D + t * t in column order from +0.0;  dist = sqrt(D)
//   pair distance, cosine      p = p + x_it * x_jt in column order from +0.0;  q_i = sqrt(the x_it * x_it by the same chain), once per row;
//                              c = p / (q_i * q_j), 0 where either norm is 0;  dist = 1 - c, 0 where that is not above 0
//   per (row i, cluster c)     the dist of the members j != i of c in ascending row order from +0.0
//   per row                    a = sum_own / (size_own - 1);  b = the smallest sum_c / size_c over the non-empty c != own, the first among equals over
//                              ascending c, nearest = that c;  s = (b - a) / max(a, b);  s = 0 for size_own == 1 (then a = 0 too), max(a, b) == 0
//                              or no other member (then b = 0, nearest = -1);  a row with a label outside [0, k): s = a = b = 0, nearest = -1
//   cluster_mean[c]            the members' s in ascending row order from +0.0, divided by sizes[c]; 0 for an empty cluster
//   mean                       launch_chain_mean over s (chain.hip)
//
// Kernels:
//   (kmeans.hip, wide_group)   every block of 512 rows sorted by (label, row), and the block's (label, first position) segments
//   sil_count_kernel           cnt[c][block] = the length of cluster c's segment in the block (cnt zeroed before)
//   sil_prefix_kernel          thread = cluster: cnt[c][.] becomes its exclusive prefix over the blocks, sizes[c] the total
//   sil_start_kernel           ONE workgroup: start[k + 1], the exclusive prefix of sizes
//   sil_scatter_kernel         workgroup = block: position start[c] + cnt[c][block] + (place in the segment) of the global order receives the row -
//                              a stable counting sort by label: order[start[c] .. start[c + 1]) are the members of c in ascending row order
//   sil_norm_kernel            thread = row: q_i (cosine only)
//   sil_pair_kernel<METRIC>    workgroup = SL_T = 64 consecutive rows i in natural order; it streams the grouped rows j through order in tiles of 64.
//                              Per chunk of SL_DC = 16 columns both tiles go to LDS as doubles, column-major; thread = 4 x 4 of the 64 x 64 pairs, its
//                              16 chains in registers across the column loop (four 16-byte LDS reads per column against 48 fp64 operations); the
//                              next chunk's floats are in flight in registers meanwhile.  The finished distances go to LDS; then thread r < 64
//                              walks the 64 entries of row r in order: stretch by stretch of one cluster it adds to the running sum (eight entries
//                              in flight), and closes the cluster where start[] says it ends - inside a tile, at its edge, or many tiles later -
//                              updating a, or b and nearest, in registers.  64 adds per row and tile against 64 * 3 d operations.  160 registers
//                              and 49 KB of LDS: three workgroups per CU, which the barriers and the one-wave walk need (measured: a column loop
//                              unrolled by hand to 178 registers, two workgroups per CU, ran 1.16 to 1.22x slower; the walk with a test per entry 1.03 to
//                              1.16x slower)
//   sil_cluster_mean_kernel    workgroup = cluster: its members' s staged 512 at a time, thread 0 adds them in order
//   (chain.hip, launch_chain_mean)  mean
#include "kernels.h"

namespace gr {

constexpr int SL_T = 64;                // rows of a tile, on both sides of the pair
constexpr int SL_DC = 16;               // columns per LDS stage: 2 x 8.4 KB of operands + 32 KB of distances = 49 KB, three workgroups per CU
constexpr int SL_LD = SL_T + 2;         // leading dimension of a staged column: 16-byte aligned groups of 4 rows, columns 4 banks apart
constexpr int SL_KMAX = 4096, SL_DMAX = 256;

__global__ __launch_bounds__(256) void sil_count_kernel(int segs, const int* __restrict__ seg_label, const int* __restrict__ seg_start,
                                                         const int* __restrict__ nseg, const int* __restrict__ nvalid, long nblk, int* __restrict__ cnt) {
  const long b = blockIdx.x;
  const int ns = nseg[b], nv = nvalid[b];
  for (int sg = threadIdx.x; sg < ns; sg += 256) {
    const int lo = seg_start[b * segs + sg], hi = sg + 1 < ns ? seg_start[b * segs + sg + 1] : nv;
    cnt[(long)seg_label[b * segs + sg] * nblk + b] = hi - lo;
  }
}

__global__ void sil_prefix_kernel(int* __restrict__ cnt, long nblk, int k, int* __restrict__ sizes) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  int run = 0;
  for (long b = 0; b < nblk; ++b) { const int v = cnt[(long)c * nblk + b]; cnt[(long)c * nblk + b] = run; run += v; }
  sizes[c] = run;
}

__global__ __launch_bounds__(256) void sil_start_kernel(const int* __restrict__ sizes, int k, int* __restrict__ start) {
  __shared__ int part[257];
  const int tid = threadIdx.x, per = (k + 255) / 256, lo = min(k, tid * per), hi = min(k, lo + per);
  int run = 0;
  for (int c = lo; c < hi; ++c) run += sizes[c];
  part[tid + 1] = run;
  __syncthreads();
  if (tid == 0) { part[0] = 0; for (int t = 1; t <= 256; ++t) part[t] += part[t - 1]; }
  __syncthreads();
  run = part[tid];
  for (int c = lo; c < hi; ++c) { start[c] = run; run += sizes[c]; }
  if (tid == 255) start[k] = part[256];
}

__global__ __launch_bounds__(256) void sil_scatter_kernel(int segs, const int* __restrict__ seg_label, const int* __restrict__ seg_start,
                                                           const int* __restrict__ nseg, const int* __restrict__ nvalid, const int* __restrict__ border,
                                                           long nblk, const int* __restrict__ cnt, const int* __restrict__ start, int* __restrict__ order) {
  const long b = blockIdx.x;
  const int ns = nseg[b], nv = nvalid[b];
  const int* ss = seg_start + b * segs;
  for (int i = threadIdx.x; i < nv; i += 256) {
    int lo = 0, hi = ns - 1;                                            // the last segment that starts at or before i
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ss[mid] <= i) lo = mid; else hi = mid - 1; }
    const int c = seg_label[b * segs + lo];
    order[start[c] + cnt[(long)c * nblk + b] + (i - ss[lo])] = border[b * ROWS_PER_BLOCK + i];
  }
}

__global__ void sil_norm_kernel(const float* __restrict__ x, long n, int d, double* __restrict__ qn) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p = 0.0;
  for (int t = 0; t < d; ++t) { const double v = (double)x[i * d + t]; p = p + v * v; }
  qn[i] = sqrt(p);
}

// An entry's place in a staged column of the grouped rows: entries 4 tx .. 4 tx + 3 are one thread's, read as two 16-byte halves; the halves of the
// threads tx >= 8 are swapped, so that the 16 threads of a read group cover all 64 banks once (tx and tx + 8 would meet on the same 4 otherwise)
__device__ __forceinline__ int sl_swz(int r) { return r ^ ((r >> 4) & 2); }
__device__ __forceinline__ void sl_operands(const double (*As)[SL_LD], const double (*Bs)[SL_LD], int t, int tx, int ty, double* a, double* b) {
  const int sw = (tx >> 2) & 2;                                         // sl_swz of 4 tx: where the thread's first half lies
  const double2 a01 = *reinterpret_cast<const double2*>(&As[t][4 * ty]), a23 = *reinterpret_cast<const double2*>(&As[t][4 * ty + 2]);
  const double2 b01 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + sw]), b23 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + (sw ^ 2)]);
  a[0] = a01.x; a[1] = a01.y; a[2] = a23.x; a[3] = a23.y;
  b[0] = b01.x; b[1] = b01.y; b[2] = b23.x; b[3] = b23.y;
}
template <int METRIC> __device__ __forceinline__ void sl_pair(double (&acc)[4][4], const double* a, const double* b) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (METRIC == 0) { const double df = a[u] - b[v]; acc[u][v] = acc[u][v] + df * df; }
      else acc[u][v] = acc[u][v] + a[u] * b[v];
    }
}

template <int METRIC>
__global__ __launch_bounds__(256) void sil_pair_kernel(const float* __restrict__ x, long n, int d, const int* __restrict__ labels, int k,
                                                        const int* __restrict__ order, const int* __restrict__ start, const double* __restrict__ qn,
                                                        double* __restrict__ s_out, double* __restrict__ a_out, double* __restrict__ b_out,
                                                        int* __restrict__ nearest_out) {
  __shared__ __attribute__((aligned(16))) double As[SL_DC][SL_LD], Bs[SL_DC][SL_LD];
  __shared__ __attribute__((aligned(16))) double Ds[SL_T][SL_T];        // [j of the tile][row of the workgroup]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;            // thread = rows 4 ty .. 4 ty + 3 x tile entries 4 tx .. 4 tx + 3:
  const long i0 = (long)blockIdx.x * SL_T;                              // a wave reads 4 row addresses (broadcast) and the 64 entries, 16 bytes per lane
  const int m = start[k];                                               // rows with a cluster
  // the walking thread's row (tid < 64)
  const long iw = i0 + tid;
  const int own_raw = (tid < SL_T && iw < n) ? labels[iw] : -1;
  const int own = (own_raw >= 0 && own_raw < k) ? own_raw : -1;
  double run = 0.0, own_sum = 0.0, bmin = 0.0;
  int nearest = -1;
  int cur = 0;                                                          // the cluster the walk is in: the first non-empty one
  while (cur < k && start[cur + 1] == start[cur]) ++cur;
  int end = cur < k ? start[cur + 1] : -1;
  // the loader's role: column lc of the chunk, rows lr + LP q of the tile - SL_DC consecutive lanes read SL_DC consecutive floats of a row
  constexpr int LP = 256 / SL_DC, LQ = SL_T / LP;
  const int lc = tid % SL_DC, lr = tid / SL_DC;

  for (int j0 = 0; j0 < m; j0 += SL_T) {
    const int nj = min(SL_T, m - j0);
    int jl[LQ], jb[4];                                                  // the tile's rows: the ones this thread loads, the ones it pairs
#pragma unroll
    for (int q = 0; q < LQ; ++q) jl[q] = lr + LP * q < nj ? order[j0 + lr + LP * q] : -1;
#pragma unroll
    for (int v = 0; v < 4; ++v) jb[v] = 4 * tx + v < nj ? order[j0 + 4 * tx + v] : -1;
    float fa[LQ], fb[LQ];                                               // the next chunk, in flight while this one is paired
    auto fetch = [&](int c0) {
      const bool in = c0 + lc < d;
#pragma unroll
      for (int q = 0; q < LQ; ++q) {
        const long ia = i0 + lr + LP * q;
        fa[q] = (in && ia < n) ? x[ia * d + c0 + lc] : 0.f;
        fb[q] = (in && jl[q] >= 0) ? x[(long)jl[q] * d + c0 + lc] : 0.f;
      }
    };
    fetch(0);
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int c0 = 0; c0 < d; c0 += SL_DC) {
      const int dc = min(SL_DC, d - c0);
      __syncthreads();                                                  // the stage before this one has been read
#pragma unroll
      for (int q = 0; q < LQ; ++q) { As[lc][lr + LP * q] = (double)fa[q]; Bs[lc][sl_swz(lr + LP * q)] = (double)fb[q]; }
      __syncthreads();
      if (c0 + SL_DC < d) fetch(c0 + SL_DC);
      for (int t = 0; t < dc; ++t) {
        double a[4], b[4];
        sl_operands(As, Bs, t, tx, ty, a, b);
        sl_pair<METRIC>(acc, a, b);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const double qj = (METRIC == 1 && jb[v] >= 0) ? qn[jb[v]] : 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long i = i0 + 4 * ty + u;
        double dist;
        if (METRIC == 0) dist = sqrt(acc[u][v]);
        else {
          const double qi = i < n ? qn[i] : 0.0;
          const double den = qi * qj;
          const double c = (qi == 0.0 || qj == 0.0) ? 0.0 : acc[u][v] / den;
          const double e = 1.0 - c;
          dist = e > 0.0 ? e : 0.0;
        }
        if (jb[v] < 0 || i >= n || (long)jb[v] == i) dist = 0.0;        // a row is not its own neighbour: +0.0 leaves the chain's bits
        Ds[4 * tx + v][4 * ty + u] = dist;
      }
    }
    __syncthreads();
    if (tid < SL_T) {
      int jj = 0;
      while (jj < nj) {                                                 // the stretch of the tile that lies in cluster cur (the same in every thread)
        const int hi = min(nj, end - j0);
        for (; jj + 8 <= hi; jj += 8) {                                 // eight entries in flight, added in order
          double e[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) e[u] = Ds[jj + u][tid];
#pragma unroll
          for (int u = 0; u < 8; ++u) run = run + e[u];
        }
        for (; jj < hi; ++jj) run = run + Ds[jj][tid];
        if (j0 + hi == end) {                                           // cluster cur ends here
          const int size = end - start[cur];
          if (cur == own) own_sum = run;
          else {
            const double mc = run / (double)size;
            if (nearest < 0 || mc < bmin) { bmin = mc; nearest = cur; }
          }
          run = 0.0;
          ++cur;
          while (cur < k && start[cur + 1] == start[cur]) ++cur;
          end = cur < k ? start[cur + 1] : -1;
        }
      }
    }
  }
  if (tid < SL_T && iw < n) {
    double a = 0.0, b = 0.0, sv = 0.0;
    if (own >= 0) {
      const int size = start[own + 1] - start[own];
      if (size > 1) a = own_sum / (double)(size - 1);
      if (nearest >= 0) {
        b = bmin;
        const double mx = a > b ? a : b;
        if (size > 1 && mx != 0.0) sv = (b - a) / mx;
      }
    } else nearest = -1;
    s_out[iw] = sv;
    if (a_out) a_out[iw] = a;
    if (b_out) b_out[iw] = b;
    if (nearest_out) nearest_out[iw] = nearest;
  }
}

__global__ __launch_bounds__(64) void sil_cluster_mean_kernel(const double* __restrict__ sv, const int* __restrict__ order, const int* __restrict__ start,
                                                               double* __restrict__ cluster_mean) {
  __shared__ double v[ROWS_PER_BLOCK];
  const int c = blockIdx.x, lo = start[c], hi = start[c + 1];
  double s = 0.0;
  for (int p0 = lo; p0 < hi; p0 += ROWS_PER_BLOCK) {
    const int np = min(ROWS_PER_BLOCK, hi - p0);
    __syncthreads();
    for (int e = threadIdx.x; e < np; e += 64) v[e] = sv[order[p0 + e]];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int e = 0; e < np; ++e) s = s + v[e];
  }
  if (threadIdx.x == 0) cluster_mean[c] = hi > lo ? s / (double)(hi - lo) : 0.0;
}

// ------------------------------------------------------------------ launcher
// the index of the labelling (wide_index_bytes), then ints: cnt [k][ceil(n / 512)], start [k + 1], order [n]; doubles: q [n], the block partials of
// the mean [ceil(n / 512)]
size_t silhouette_workspace_bytes(long n, int k) {
  const size_t nblk = (size_t)row_blocks(n);
  return wide_index_bytes(n, k) + sizeof(int) * ((size_t)k * nblk + (size_t)k + 1 + (size_t)n) + sizeof(double) * ((size_t)n + nblk) + 8 * 256;
}

int launch_silhouette(const float* x, long n, int d, const int* labels, int k, int metric, double* s_out, double* a_out, double* b_out, int* nearest,
                      double* cluster_mean, int* sizes, double* mean, void* workspace, hipStream_t s) {
  if (n < 2 || n > SIL_MAX_N || d < 1 || d > SL_DMAX || k < 1 || k > SL_KMAX || (metric != 0 && metric != 1)) return 1;
  const long nblk = row_blocks(n);
  char* ws = static_cast<char*>(workspace);
  const WideIndex ix = wide_index_carve(ws, n, k);
  auto take = [&](size_t bytes) { char* p = ws; ws += (bytes + 255) / 256 * 256; return p; };
  int* cnt = reinterpret_cast<int*>(take(sizeof(int) * (size_t)k * nblk));
  int* start = reinterpret_cast<int*>(take(sizeof(int) * ((size_t)k + 1)));
  int* order = reinterpret_cast<int*>(take(sizeof(int) * (size_t)n));
  double* qn = reinterpret_cast<double*>(take(sizeof(double) * (size_t)n));
  double* part = reinterpret_cast<double*>(take(sizeof(double) * (size_t)nblk));
  const int segs = wide_index_segs(k);
  wide_group(labels, n, k, ix, s);
  { KtScope kt("sil_group_kernels", 0.0, 8.0 * k * nblk + 12.0 * n, s);
    (void)hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)k * nblk, s);
    hipLaunchKernelGGL(sil_count_kernel, dim3((unsigned)nblk), dim3(256), 0, s, segs, ix.seg_label, ix.seg_start, ix.nseg, ix.nvalid, nblk, cnt);
    hipLaunchKernelGGL(sil_prefix_kernel, dim3((k + 63) / 64), dim3(64), 0, s, cnt, nblk, k, sizes);
    hipLaunchKernelGGL(sil_start_kernel, dim3(1), dim3(256), 0, s, sizes, k, start);
    hipLaunchKernelGGL(sil_scatter_kernel, dim3((unsigned)nblk), dim3(256), 0, s, segs, ix.seg_label, ix.seg_start, ix.nseg, ix.nvalid, ix.order, nblk,
                       cnt, start, order); }
  if (metric == 1) {
    KtScope kt("sil_norm_kernel", 2.0 * n * d, 4.0 * n * d, s);
    hipLaunchKernelGGL(sil_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, d, qn);
  }
  const unsigned grid = (unsigned)((n + SL_T - 1) / SL_T);
  { KtScope kt(metric ? "sil_pair_kernel<cosine>" : "sil_pair_kernel<euclidean>", (metric ? 2.0 : 3.0) * n * n * d, 4.0 * n * d * grid, s);
    if (metric) hipLaunchKernelGGL(sil_pair_kernel<1>, dim3(grid), dim3(256), 0, s, x, n, d, labels, k, order, start, qn, s_out, a_out, b_out, nearest);
    else hipLaunchKernelGGL(sil_pair_kernel<0>, dim3(grid), dim3(256), 0, s, x, n, d, labels, k, order, start, qn, s_out, a_out, b_out, nearest); }
  { KtScope kt("sil_cluster_mean_kernel", (double)n, 12.0 * n, s);
    hipLaunchKernelGGL(sil_cluster_mean_kernel, dim3(k), dim3(64), 0, s, s_out, order, start, cluster_mean); }
  launch_chain_mean(s_out, n, part, mean, "sil_mean_kernels", s);
  return 0;
}

}  // namespace gr
