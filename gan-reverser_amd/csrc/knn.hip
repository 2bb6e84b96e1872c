// knn.hip — the exact k-nearest-neighbour graph of a device table [n x d], n <= 262144, d <= 256, k <= min(n - 1, 128), built and left on the device
// (gr_knn_dev), and what is read off such a graph: local outlier factors (gr_lof_dev) and the overlap of two graphs (gr_knn_overlap_dev).  New: the
// reference has no counterpart; its README's anomaly section is what the outlier factor answers without a model of the table.
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/knn_paths.py; this file is compiled without FMA contraction (Makefile),
// so every multiply and add below rounds on its own.  Everything past the loads is fp64.  No floating-point atomics, no grid barrier: every result is a
// function of the inputs alone.
//
// Operation by operation (all fp64; the pair distances are silhouette.hip's, bit for bit):
//   pair distance, euclidean   t = x_it - x_jt;  D = D + t * t in column order from +0.0;  dist = sqrt(D)
//   pair distance, cosine      p = p + x_it * x_jt in column order from +0.0;  q_i = sqrt(the x_it * x_it by the same chain), once per row;
//                              c = p / (q_i * q_j), 0 where either norm is 0;  dist = 1 - c, 0 where that is not above 0
//   row i's list               the k rows j != i of smallest dist, by (dist ascending, j ascending): j is visited in ascending order and enters the
//                              list only where dist < the list's current k-th dist (any dist while the list is short), behind its equals
//   lrd, lof                   kdist_j = dist[j][k - 1];  reach = max(kdist_j, dist[i][p]);  m_i = (the k reach in list order from +0.0) / k;
//                              lrd_i = 1 / (m_i + 1e-10);  lof_i = ((the neighbours' lrd in list order from +0.0) / k) / lrd_i
//   overlap                    count_i = the entries of a's row i that occur in b's row i;  mean = launch_chain_mean over count_i / k (chain.hip)
//
// Kernels:
//   knn_norm_kernel            thread = row: q_i (cosine only)
//   knn_pair_kernel<METRIC>    sil_pair_kernel's pair part: workgroup = KN_T = 64 consecutive rows i; the rows j stream by in natural ascending order in
//                              tiles of 64.  Per chunk of KN_DC = 16 columns both tiles go to LDS as doubles, column-major, the j side swizzled; thread =
//                              4 x 4 of the 64 x 64 pairs, its 16 chains in registers across the column loop; the next chunk's floats are in flight in
//                              registers meanwhile.  The finished distances go to LDS - +inf for a pair that is none (j = i, j >= n, i >= n) - then
//                              thread r < 64 walks the 64 entries of row r in order, eight loads in flight, against the list's k-th distance, which it
//                              keeps in a register (+inf while the list is short): one compare per entry, and an insertion on a hit.  Because j
//                              ascends, the strict < sends a tie to the lower row.
//                              The lists are the output rows themselves (idx [n x k], dist [n x k]): only the thread that owns a row reads or writes
//                              it, and it stays cache-resident between hits.  In LDS the lists would cost 12 bytes x 64 rows x k - 15 KB at k = 20 but
//                              96 KB at k = 128, next to the 49 KB of the pair part: one workgroup per CU instead of three, and the barriers and the
//                              one-wave walk have nothing to hide behind (silhouette.hip measured two per CU at 1.16 to 1.22x).  An insertion reads
//                              the list from its end eight entries at a time (independent loads), moves up the ones that are larger and stops at the
//                              first group that holds one that is not: ceil((moves + 1) / 8) round trips to the cache.
//                              Cost of the walk: for rows in random order entry j enters with probability k / j, about k ln(n / k) insertions per
//                              row of k / 2 moves on average, nearly all of them in the first tiles.  The adversarial case is a table sorted so that
//                              every later row is nearer (to row 0, say): every entry enters at the head, n k list moves for that row.
//   knn_lrd_kernel, knn_lof_kernel   thread = row: the two chains above (two launches: lof reads every row's lrd)
//   knn_overlap_kernel         thread = row: k x k compares, count and count / k
//   (chain.hip, launch_chain_mean)  the overlap's mean
#include "kernels.h"

namespace gr {

constexpr int KN_T = 64;                // rows of a tile, on both sides of the pair
constexpr int KN_DC = 16;               // columns per LDS stage: 2 x 8.4 KB of operands + 32 KB of distances = 49 KB, three workgroups per CU
constexpr int KN_LD = KN_T + 2;         // leading dimension of a staged column: 16-byte aligned groups of 4 rows, columns 4 banks apart
constexpr int KN_DMAX = 256, KN_KMAX = 128;
constexpr int KN_G = 8;                 // list entries an insertion reads at a time

__global__ void knn_norm_kernel(const float* __restrict__ x, long n, int d, double* __restrict__ qn) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p = 0.0;
  for (int t = 0; t < d; ++t) { const double v = (double)x[i * d + t]; p = p + v * v; }
  qn[i] = sqrt(p);
}

// silhouette.hip's staged layout (sl_swz, sl_operands, sl_pair), restated here so that that file's object stays what it was: entries 4 tx .. 4 tx + 3
// of a staged column are one thread's, read as two 16-byte halves; the halves of the threads tx >= 8 are swapped, so that the 16 threads of a read
// group cover all 64 banks once
__device__ __forceinline__ int kn_swz(int r) { return r ^ ((r >> 4) & 2); }
__device__ __forceinline__ void kn_operands(const double (*As)[KN_LD], const double (*Bs)[KN_LD], int t, int tx, int ty, double* a, double* b) {
  const int sw = (tx >> 2) & 2;
  const double2 a01 = *reinterpret_cast<const double2*>(&As[t][4 * ty]), a23 = *reinterpret_cast<const double2*>(&As[t][4 * ty + 2]);
  const double2 b01 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + sw]), b23 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + (sw ^ 2)]);
  a[0] = a01.x; a[1] = a01.y; a[2] = a23.x; a[3] = a23.y;
  b[0] = b01.x; b[1] = b01.y; b[2] = b23.x; b[3] = b23.y;
}
template <int METRIC> __device__ __forceinline__ void kn_pair(double (&acc)[4][4], const double* a, const double* b) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (METRIC == 0) { const double df = a[u] - b[v]; acc[u][v] = acc[u][v] + df * df; }
      else acc[u][v] = acc[u][v] + a[u] * b[v];
    }
}

// (e, j) enters the sorted list il / dl, which holds cnt <= k entries and keeps at most k: behind every entry that is not larger.  The caller has
// checked e < dl[k - 1] when cnt == k.  -> the list's k-th distance afterwards, +inf while it is short
__device__ __forceinline__ double kn_insert(int* __restrict__ il, double* __restrict__ dl, int& cnt, int k, double e, int j) {
  int q = cnt < k ? cnt : k - 1;                                        // the free slot: past the end, or the last entry's, which leaves
  double last = e;                                                      // what slot k - 1 holds afterwards, once the list is full
  bool first = true;
  while (q > 0) {
    const int g = min(KN_G, q);
    double dv[KN_G]; int iv[KN_G];
#pragma unroll
    for (int u = 0; u < KN_G; ++u)
      if (u < g) { dv[u] = dl[q - 1 - u]; iv[u] = il[q - 1 - u]; }
    int moved = 0;
#pragma unroll
    for (int u = 0; u < KN_G; ++u)
      if (u < g && u == moved && dv[u] > e) { dl[q - u] = dv[u]; il[q - u] = iv[u]; ++moved; }
    if (first && moved > 0) last = dv[0];
    first = false;
    q -= moved;
    if (moved < KN_G) break;
  }
  dl[q] = e; il[q] = j;
  if (cnt < k) ++cnt;
  return cnt == k ? last : __builtin_huge_val();
}

template <int METRIC>
__global__ __launch_bounds__(256) void knn_pair_kernel(const float* __restrict__ x, long n, int d, int k, const double* __restrict__ qn,
                                                        int* __restrict__ idx_out, double* __restrict__ dist_out) {
  __shared__ __attribute__((aligned(16))) double As[KN_DC][KN_LD], Bs[KN_DC][KN_LD];
  __shared__ __attribute__((aligned(16))) double Ds[KN_T][KN_T];        // [j of the tile][row of the workgroup]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;            // thread = rows 4 ty .. 4 ty + 3 x tile entries 4 tx .. 4 tx + 3
  const long i0 = (long)blockIdx.x * KN_T;
  const double inf = __builtin_huge_val();
  // the walking thread's row (tid < 64) and its list
  const long iw = i0 + tid;
  const bool walks = tid < KN_T && iw < n;
  int* il = idx_out + (walks ? iw : 0) * k;
  double* dl = dist_out + (walks ? iw : 0) * k;
  int cnt = 0;
  double kth = inf;
  // the loader's role: column lc of the chunk, rows lr + LP q of the tile - KN_DC consecutive lanes read KN_DC consecutive floats of a row
  constexpr int LP = 256 / KN_DC, LQ = KN_T / LP;
  const int lc = tid % KN_DC, lr = tid / KN_DC;

  for (long j0 = 0; j0 < n; j0 += KN_T) {
    float fa[LQ], fb[LQ];                                               // the next chunk, in flight while this one is paired
    auto fetch = [&](int c0) {
      const bool in = c0 + lc < d;
#pragma unroll
      for (int q = 0; q < LQ; ++q) {
        const long ia = i0 + lr + LP * q, jb = j0 + lr + LP * q;
        fa[q] = (in && ia < n) ? x[ia * d + c0 + lc] : 0.f;
        fb[q] = (in && jb < n) ? x[jb * d + c0 + lc] : 0.f;
      }
    };
    fetch(0);
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int c0 = 0; c0 < d; c0 += KN_DC) {
      const int dc = min(KN_DC, d - c0);
      __syncthreads();                                                  // the stage before this one has been read (and the tile before this one walked)
#pragma unroll
      for (int q = 0; q < LQ; ++q) { As[lc][lr + LP * q] = (double)fa[q]; Bs[lc][kn_swz(lr + LP * q)] = (double)fb[q]; }
      __syncthreads();
      if (c0 + KN_DC < d) fetch(c0 + KN_DC);
      for (int t = 0; t < dc; ++t) {
        double a[4], b[4];
        kn_operands(As, Bs, t, tx, ty, a, b);
        kn_pair<METRIC>(acc, a, b);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long j = j0 + 4 * tx + v;
      const double qj = (METRIC == 1 && j < n) ? qn[j] : 0.0;
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
        if (j >= n || i >= n || j == i) dist = inf;                     // no pair: it never passes the walk's test
        Ds[4 * tx + v][4 * ty + u] = dist;
      }
    }
    __syncthreads();
    if (walks) {
      for (int jj = 0; jj < KN_T; jj += 8) {                            // eight entries in flight, tested in order
        double e[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) e[u] = Ds[jj + u][tid];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (e[u] < kth) kth = kn_insert(il, dl, cnt, k, e[u], (int)(j0 + jj + u));
      }
    }
  }
}

__global__ void knn_lrd_kernel(const int* __restrict__ idx, const double* __restrict__ dist, long n, int k, double* __restrict__ lrd) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double m = 0.0;
  for (int p = 0; p < k; ++p) {
    const double kd = dist[(long)idx[i * k + p] * k + k - 1], own = dist[i * k + p];
    m = m + (kd > own ? kd : own);
  }
  m = m / (double)k;
  lrd[i] = 1.0 / (m + 1e-10);
}

__global__ void knn_lof_kernel(const int* __restrict__ idx, const double* __restrict__ lrd, long n, int k, double* __restrict__ lof) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int p = 0; p < k; ++p) s = s + lrd[idx[i * k + p]];
  s = s / (double)k;
  lof[i] = s / lrd[i];
}

__global__ void knn_overlap_kernel(const int* __restrict__ a, const int* __restrict__ b, long n, int k, int* __restrict__ count, double* __restrict__ share) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int c = 0;
  for (int p = 0; p < k; ++p) {
    const int want = a[i * k + p];
    bool found = false;
    for (int q = 0; q < k; ++q) found = found || b[i * k + q] == want;
    c += found ? 1 : 0;
  }
  count[i] = c;
  share[i] = (double)c / (double)k;
}

// ------------------------------------------------------------------ launchers
size_t knn_workspace_bytes(long n) { return sizeof(double) * (size_t)n + 256; }      // the norms (cosine)

int launch_knn(const float* x, long n, int d, int k, int metric, int* idx_out, double* dist_out, void* workspace, hipStream_t s) {
  if (n < 2 || n > KNN_MAX_N || d < 1 || d > KN_DMAX || k < 1 || k > KN_KMAX || k > n - 1 || (metric != 0 && metric != 1)) return 1;
  double* qn = static_cast<double*>(workspace);
  if (metric == 1) {
    KtScope kt("knn_norm_kernel", 2.0 * n * d, 4.0 * n * d, s);
    hipLaunchKernelGGL(knn_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, d, qn);
  }
  const unsigned grid = (unsigned)((n + KN_T - 1) / KN_T);
  KtScope kt(metric ? "knn_pair_kernel<cosine>" : "knn_pair_kernel<euclidean>", (metric ? 2.0 : 3.0) * n * n * d, 4.0 * n * d * grid, s);
  if (metric) hipLaunchKernelGGL(knn_pair_kernel<1>, dim3(grid), dim3(256), 0, s, x, n, d, k, qn, idx_out, dist_out);
  else hipLaunchKernelGGL(knn_pair_kernel<0>, dim3(grid), dim3(256), 0, s, x, n, d, k, qn, idx_out, dist_out);
  return 0;
}

size_t lof_workspace_bytes(long n) { return sizeof(double) * (size_t)n + 256; }      // lrd, where the caller does not ask for it

int launch_lof(const int* idx, const double* dist, long n, int k, double* lrd, double* lof, void* workspace, hipStream_t s) {
  if (n < 2 || n > KNN_MAX_N || k < 1 || k > KN_KMAX || k > n - 1) return 1;
  double* r = lrd ? lrd : static_cast<double*>(workspace);
  KtScope kt("knn_lof_kernels", 3.0 * n * k, 28.0 * n * k, s);
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(knn_lrd_kernel, dim3(grid), dim3(256), 0, s, idx, dist, n, k, r);
  hipLaunchKernelGGL(knn_lof_kernel, dim3(grid), dim3(256), 0, s, idx, r, n, k, lof);
  return 0;
}

size_t knn_overlap_workspace_bytes(long n) { return chain_mean_workspace_bytes(n); }  // count / k [n], then the block partials

int launch_knn_overlap(const int* a, const int* b, long n, int k, int* count, double* mean, void* workspace, hipStream_t s) {
  if (n < 2 || n > KNN_MAX_N || k < 1 || k > KN_KMAX || k > n - 1) return 1;
  double* share = static_cast<double*>(workspace);
  { KtScope kt("knn_overlap_kernel", (double)n * k * k, 8.0 * n * k, s);
    hipLaunchKernelGGL(knn_overlap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, n, k, count, share); }
  launch_chain_mean(share, n, share + (size_t)n, mean, "knn_overlap_mean_kernels", s);
  return 0;
}

}  // namespace gr
