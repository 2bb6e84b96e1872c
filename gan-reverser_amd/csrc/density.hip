// density.hip — density-based clustering of a device table [n x d], n <= 262144, d <= 256: the eps-neighbourhood graph as a bitmap, built and left on
// the device (gr_eps_graph_dev), and DBSCAN's labels read off such a bitmap (gr_dbscan_dev).  New: the reference has no counterpart; its README
// asks whether "other clustering methods would produce better results" - this is the one that finds the cluster count itself, follows groups of any
// shape and calls the rows that belong nowhere noise.
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/density_paths.py; this file is compiled without FMA contraction
// (Makefile), so every multiply and add below rounds on its own.  Everything past the loads is fp64.  No floating-point atomics, no grid barrier.
//
// Operation by operation (all fp64; the pair distances are silhouette.hip's and knn.hip's, bit for bit):
//   pair distance, euclidean   t = x_it - x_jt;  D = D + t * t in column order from +0.0;  dist = sqrt(D)
//   pair distance, cosine      p = p + x_it * x_jt in column order from +0.0;  q_i = sqrt(the x_it * x_it by the same chain), once per row;
//                              c = p / (q_i * q_j), 0 where either norm is 0;  dist = 1 - c, 0 where that is not above 0
//   bit j of row i             dist <= eps; always 1 for j = i; 0 for j >= n.  The chain is symmetric in i and j (a - b and b - a square to the same
//                              bits, the product commutes), so the bitmap is
//   count_i                    the popcount of row i
//   core_i                     count_i >= min_pts
//   label, core rows           the smallest core row of the row's connected component under the bitmap restricted to core rows
//   label, other rows          the smallest such root among the row's core neighbours; -1 without a core neighbour
//   cluster numbers            the roots' ranks in ascending row order
//
// Kernels:
//   eps_norm_kernel            thread = row: q_i (cosine only)
//   eps_pair_kernel<METRIC>    sil_pair_kernel's / knn_pair_kernel's pair part: workgroup = EP_T = 64 consecutive rows i; the rows j stream by in tiles of
//                              64 - one output word per row.  Per chunk of EP_DC = 16 columns both tiles go to LDS as doubles, column-major, the j
//                              side swizzled; thread = 4 x 4 of the 64 x 64 pairs, its 16 chains in registers across the column loop; the next chunk's
//                              floats are in flight in registers meanwhile.  The 16 threads that share a ty are 16 adjacent lanes of one wave and
//                              hold the 64 compare results of their four rows, four bits each: per row the bits go to their place in the word's
//                              low or high half (tx < 8, tx >= 8), three xor-shuffles OR the eight lanes of a half together, a fourth fetches the
//                              other half, and lane tx = u < 4 stores the word of row 4 ty + u and adds its popcount to a register.  No LDS beyond the
//                              two operand stages (16.9 KB): the registers decide the residency.
//   db_core_kernel             thread = row: core flag, label = the row itself (n for a row that is not core), and by __ballot the packed core mask
//   db_round_kernel            wave = core row: the row's words ANDed with the core mask, 64 consecutive words per step, m = the smallest label among
//                              the core neighbours; where m < label[i]: atomicMin(label[label[i]], m), atomicMin(label[i], m), changed = 1
//   db_compress_kernel         thread = core row: label[i] = the fixed point of label[label[...]].  label[x] <= x always, so the walk descends strictly
//                              and ends at a row with label[r] = r; such rows are not written during the walk, so the result does not depend on the order
//   db_border_kernel           wave = row that is not core: the same scan; the smallest root among its core neighbours, or none
//   db_rank_kernel             ONE workgroup: rank[i] = the number of roots below row i (exclusive scan of the flags label[i] == i), n_clusters
//   db_label_kernel            thread = row: the cluster number of its root, -1 without one; the core flag
// The host repeats (round, compress) until a round changes nothing: one stream wait per round to read the changed word (ops.hip).  Plain min-label
// propagation alone carries the smallest row of a component one edge per round, so n - 1 rounds always suffice and the n-th changes nothing: the cap.
#include "kernels.h"

namespace gr {

constexpr int EP_T = 64;                // rows of a tile, on both sides of the pair: one 64-bit word per row and tile
constexpr int EP_DC = 16;               // columns per LDS stage: 2 x 8.4 KB of operands
constexpr int EP_LD = EP_T + 2;         // leading dimension of a staged column: 16-byte aligned groups of 4 rows, columns 4 banks apart
constexpr int EP_DMAX = 256;

__global__ void eps_norm_kernel(const float* __restrict__ x, long n, int d, double* __restrict__ qn) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p = 0.0;
  for (int t = 0; t < d; ++t) { const double v = (double)x[i * d + t]; p = p + v * v; }
  qn[i] = sqrt(p);
}

// silhouette.hip's staged layout (sl_swz, sl_operands, sl_pair), restated here as knn.hip restates it, so that those files' objects stay what they
// were: entries 4 tx .. 4 tx + 3 of a staged column are one thread's, read as two 16-byte halves; the halves of the threads tx >= 8 are swapped, so
// that the 16 threads of a read group cover all 64 banks once
__device__ __forceinline__ int ep_swz(int r) { return r ^ ((r >> 4) & 2); }
__device__ __forceinline__ void ep_operands(const double (*As)[EP_LD], const double (*Bs)[EP_LD], int t, int tx, int ty, double* a, double* b) {
  const int sw = (tx >> 2) & 2;
  const double2 a01 = *reinterpret_cast<const double2*>(&As[t][4 * ty]), a23 = *reinterpret_cast<const double2*>(&As[t][4 * ty + 2]);
  const double2 b01 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + sw]), b23 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + (sw ^ 2)]);
  a[0] = a01.x; a[1] = a01.y; a[2] = a23.x; a[3] = a23.y;
  b[0] = b01.x; b[1] = b01.y; b[2] = b23.x; b[3] = b23.y;
}
template <int METRIC> __device__ __forceinline__ void ep_pair(double (&acc)[4][4], const double* a, const double* b) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (METRIC == 0) { const double df = a[u] - b[v]; acc[u][v] = acc[u][v] + df * df; }
      else acc[u][v] = acc[u][v] + a[u] * b[v];
    }
}

template <int METRIC>
__global__ __launch_bounds__(256) void eps_pair_kernel(const float* __restrict__ x, long n, int d, double eps, const double* __restrict__ qn,
                                                        unsigned long long* __restrict__ adj, int* __restrict__ count_out) {
  __shared__ __attribute__((aligned(16))) double As[EP_DC][EP_LD], Bs[EP_DC][EP_LD];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;            // thread = rows 4 ty .. 4 ty + 3 x tile entries 4 tx .. 4 tx + 3
  const long i0 = (long)blockIdx.x * EP_T;
  const long words = (n + 63) / 64;
  // the storing lane's row (tx < 4): row 4 ty + tx of the tile
  const long is = i0 + 4 * ty + tx;
  const bool stores = tx < 4 && is < n;
  int cnt = 0;
  // the loader's role: column lc of the chunk, rows lr + LP q of the tile - EP_DC consecutive lanes read EP_DC consecutive floats of a row
  constexpr int LP = 256 / EP_DC, LQ = EP_T / LP;
  const int lc = tid % EP_DC, lr = tid / EP_DC;

  for (long j0 = 0; j0 < n; j0 += EP_T) {
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
    for (int c0 = 0; c0 < d; c0 += EP_DC) {
      const int dc = min(EP_DC, d - c0);
      __syncthreads();                                                  // the stage before this one has been read
#pragma unroll
      for (int q = 0; q < LQ; ++q) { As[lc][lr + LP * q] = (double)fa[q]; Bs[lc][ep_swz(lr + LP * q)] = (double)fb[q]; }
      __syncthreads();
      if (c0 + EP_DC < d) fetch(c0 + EP_DC);
      for (int t = 0; t < dc; ++t) {
        double a[4], b[4];
        ep_operands(As, Bs, t, tx, ty, a, b);
        ep_pair<METRIC>(acc, a, b);
      }
    }
    unsigned half[4] = {0u, 0u, 0u, 0u};                                // per row u: this thread's four bits, at their place in their half of the word
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
        const bool bit = j < n && i < n && (dist <= eps || j == i);     // a row is in its own neighbourhood, whatever its chain says
        half[u] |= (bit ? 1u : 0u) << (4 * (tx & 7) + v);
      }
    }
    // every lane of the workgroup is here: the OR over the eight lanes of a half (lanes that differ in tx's low three bits)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      half[u] |= (unsigned)__shfl_xor((int)half[u], 1, 64);
      half[u] |= (unsigned)__shfl_xor((int)half[u], 2, 64);
      half[u] |= (unsigned)__shfl_xor((int)half[u], 4, 64);
    }
    const int su = tx & 3;
    const unsigned mine = su == 0 ? half[0] : su == 1 ? half[1] : su == 2 ? half[2] : half[3];     // tx < 4: the low half of row 4 ty + tx
    const unsigned other = (unsigned)__shfl_xor((int)mine, 8, 64);                                 // ... and its high half, from lane tx + 8
    if (stores) {
      const unsigned long long w = (unsigned long long)mine | ((unsigned long long)other << 32);
      adj[is * words + j0 / 64] = w;
      cnt += __popcll(w);
    }
  }
  if (stores) count_out[is] = cnt;
}

// ------------------------------------------------------------------ labels from a bitmap
__global__ __launch_bounds__(256) void db_core_kernel(const int* __restrict__ count, long n, int min_pts, int* __restrict__ label,
                                                       unsigned long long* __restrict__ mask) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;                  // (no lane leaves before the ballot)
  const bool core = i < n && count[i] >= min_pts;
  const unsigned long long m = __ballot(core);
  if (i < n) label[i] = core ? (int)i : (int)n;
  if ((threadIdx.x & 63) == 0 && i < n) mask[i / 64] = m;
}

// the smallest label among the core neighbours of row i, over the whole wave; n where it has none
__device__ __forceinline__ int db_scan(const unsigned long long* __restrict__ adj, const unsigned long long* __restrict__ mask,
                                       const int* label, long i, long n, long words, int lane) {
  int m = (int)n;
  for (long w = lane; w < words; w += 64) {                             // 64 consecutive words per step
    unsigned long long bits = adj[i * words + w] & mask[w];
    while (bits) {                                                      // at most 64 turns
      const int b = __ffsll((long long)bits) - 1;
      bits &= bits - 1;
      const int l = __hip_atomic_load(&label[w * 64 + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      m = min(m, l);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, 64));
  return m;
}

__global__ __launch_bounds__(256) void db_round_kernel(const unsigned long long* __restrict__ adj, const unsigned long long* __restrict__ mask, long n,
                                                        int* label, int* __restrict__ changed) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);             // wave = row: the whole wave leaves or stays
  if (i >= n || !((mask[i / 64] >> (i % 64)) & 1ull)) return;
  const long words = (n + 63) / 64;
  const int m = db_scan(adj, mask, label, i, n, words, lane);
  if (lane == 0) {
    const int li = __hip_atomic_load(&label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (m < li) {                                                       // li <= i < n: a valid row
      atomicMin(&label[li], m);
      atomicMin(&label[i], m);
      *changed = 1;
    }
  }
}

__global__ void db_compress_kernel(const unsigned long long* __restrict__ mask, long n, int* label) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !((mask[i / 64] >> (i % 64)) & 1ull)) return;
  int l = __hip_atomic_load(&label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (long step = 0; step < n; ++step) {                               // strictly descending: fewer than n steps
    const int up = __hip_atomic_load(&label[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (up == l) break;
    l = up;
  }
  __hip_atomic_store(&label[i], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void db_border_kernel(const unsigned long long* __restrict__ adj, const unsigned long long* __restrict__ mask, long n,
                                                         int* label) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n || ((mask[i / 64] >> (i % 64)) & 1ull)) return;            // core rows carry their root already; only they are read below
  const long words = (n + 63) / 64;
  const int m = db_scan(adj, mask, label, i, n, words, lane);
  if (lane == 0) label[i] = m;                                          // n: noise
}

__global__ __launch_bounds__(256) void db_rank_kernel(const int* __restrict__ label, long n, int* __restrict__ rank, int* __restrict__ n_clusters) {
  __shared__ int part[257];
  const int tid = threadIdx.x;
  const long per = (n + 255) / 256, lo = min(n, tid * per), hi = min(n, lo + per);
  int run = 0;
  for (long i = lo; i < hi; ++i) run += label[i] == (int)i ? 1 : 0;
  part[tid + 1] = run;
  __syncthreads();
  if (tid == 0) { part[0] = 0; for (int t = 1; t <= 256; ++t) part[t] += part[t - 1]; }
  __syncthreads();
  run = part[tid];
  for (long i = lo; i < hi; ++i) { rank[i] = run; run += label[i] == (int)i ? 1 : 0; }
  if (tid == 255) *n_clusters = part[256];
}

__global__ void db_label_kernel(const int* __restrict__ label, const int* __restrict__ rank, const unsigned long long* __restrict__ mask, long n,
                                int* __restrict__ labels_out, int* __restrict__ core_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = label[i];
  labels_out[i] = l < (int)n ? rank[l] : -1;
  if (core_out) core_out[i] = (int)((mask[i / 64] >> (i % 64)) & 1ull);
}

// ------------------------------------------------------------------ launchers
size_t eps_graph_workspace_bytes(long n) { return sizeof(double) * (size_t)n + 256; }  // the norms (cosine)

int launch_eps_graph(const float* x, long n, int d, double eps, int metric, unsigned long long* adj, int* count, void* workspace, hipStream_t s) {
  if (n < 2 || n > DBSCAN_MAX_N || d < 1 || d > EP_DMAX || !(eps >= 0.0) || eps > 1.7976931348623157e308 || (metric != 0 && metric != 1)) return 1;
  double* qn = static_cast<double*>(workspace);
  if (metric == 1) {
    KtScope kt("eps_norm_kernel", 2.0 * n * d, 4.0 * n * d, s);
    hipLaunchKernelGGL(eps_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, d, qn);
  }
  const unsigned grid = (unsigned)((n + EP_T - 1) / EP_T);
  KtScope kt(metric ? "eps_pair_kernel<cosine>" : "eps_pair_kernel<euclidean>", (metric ? 2.0 : 3.0) * n * n * d, 4.0 * n * d * grid + (double)n * n / 8, s);
  if (metric) hipLaunchKernelGGL(eps_pair_kernel<1>, dim3(grid), dim3(256), 0, s, x, n, d, eps, qn, adj, count);
  else hipLaunchKernelGGL(eps_pair_kernel<0>, dim3(grid), dim3(256), 0, s, x, n, d, eps, qn, adj, count);
  return 0;
}

// ints: label [n], rank [n], changed [1]; words: the core mask [ceil(n / 64)]
static size_t db_align(size_t bytes) { return (bytes + 255) / 256 * 256; }
size_t dbscan_workspace_bytes(long n) { return 2 * db_align(sizeof(int) * (size_t)n) + db_align(sizeof(int)) + db_align(8 * (size_t)((n + 63) / 64)); }

DbscanScratch dbscan_carve(void* workspace, long n) {
  char* ws = static_cast<char*>(workspace);
  auto take = [&](size_t bytes) { char* p = ws; ws += db_align(bytes); return p; };
  DbscanScratch w;
  w.label = reinterpret_cast<int*>(take(sizeof(int) * (size_t)n));
  w.rank = reinterpret_cast<int*>(take(sizeof(int) * (size_t)n));
  w.changed = reinterpret_cast<int*>(take(sizeof(int)));
  w.mask = reinterpret_cast<unsigned long long*>(take(8 * (size_t)((n + 63) / 64)));
  return w;
}

int launch_dbscan_begin(const int* count, long n, int min_pts, const DbscanScratch& w, hipStream_t s) {
  if (n < 2 || n > DBSCAN_MAX_N || min_pts < 1 || min_pts > n) return 1;
  KtScope kt("dbscan_core_kernel", (double)n, 8.0 * n, s);
  hipLaunchKernelGGL(db_core_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, count, n, min_pts, w.label, w.mask);
  return 0;
}

void launch_dbscan_round(const unsigned long long* adj, long n, const DbscanScratch& w, hipStream_t s) {
  KtScope kt("dbscan_round_kernels", (double)n * n / 64, (double)n * n / 8, s);
  (void)hipMemsetAsync(w.changed, 0, sizeof(int), s);
  hipLaunchKernelGGL(db_round_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, adj, w.mask, n, w.label, w.changed);
  hipLaunchKernelGGL(db_compress_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.mask, n, w.label);
}

void launch_dbscan_finish(const unsigned long long* adj, long n, const DbscanScratch& w, int* labels, int* core, int* n_clusters, hipStream_t s) {
  KtScope kt("dbscan_label_kernels", (double)n * n / 64, (double)n * n / 8, s);
  hipLaunchKernelGGL(db_border_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, adj, w.mask, n, w.label);
  hipLaunchKernelGGL(db_rank_kernel, dim3(1), dim3(256), 0, s, w.label, n, w.rank, n_clusters);
  hipLaunchKernelGGL(db_label_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.label, w.rank, w.mask, n, labels, core);
}

}  // namespace gr
