// mst.hip — the exact minimum spanning tree of a device table [n x d], n <= 262144, d <= 256, under the pair distance or the mutual-reachability
// distance (gr_mst_dev).  New: the reference has no counterpart; its README asks whether "other clustering methods would produce better results" -
// one such tree is the whole single-linkage dendrogram, DBSCAN*'s labels for every eps at once and, through the condensed tree (hdbscan.cpp, on the
// host), HDBSCAN's labels with no eps at all.  The tree is the n^2 d part: it is built here.
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in tests/hierarchy_paths.py; this file is compiled without FMA contraction
// (Makefile), so every multiply and add below rounds on its own.  Everything past the loads is fp64.  No floating-point atomics, no grid barrier.
//
// Operation by operation (all fp64; the pair distances are silhouette.hip's, knn.hip's and density.hip's, bit for bit):
//   pair distance, euclidean   t = x_it - x_jt;  D = D + t * t in column order from +0.0;  dist = sqrt(D)
//   pair distance, cosine      p = p + x_it * x_jt in column order from +0.0;  q_i = sqrt(the x_it * x_it by the same chain), once per row;
//                              c = p / (q_i * q_j), 0 where either norm is 0;  dist = 1 - c, 0 where that is not above 0
//   weight                     w_ij = dist; where core_i > w: core_i; where core_j > w: core_j (core_i = core[i * core_stride]; no core: dist alone).
//                              Never negative and never -0.0, so the 64-bit pattern of w orders as w does
//   edge order                 (w, min(i, j), max(i, j)) ascending: a strict total order over the n (n - 1) / 2 edges, so the minimum spanning tree is
//                              unique; the outputs hold its n - 1 edges, eu < ev, ascending by that order - a function of the inputs alone
//
// Boruvka rounds.  comp[i] is one fixed row of row i's component, its root (comp[root] = root); at the start comp[i] = i.  One round:
//   mst_pair_kernel<METRIC>    sil_pair_kernel's / knn_pair_kernel's / eps_pair_kernel's pair part: workgroup = MS_T = 64 consecutive rows i; the rows j
//                              stream by in tiles of 64.  Per chunk of MS_DC = 16 columns both tiles go to LDS as doubles, column-major, the j side
//                              swizzled; thread = 4 x 4 of the 64 x 64 pairs, its 16 chains in registers across the column loop; the next chunk's
//                              floats are in flight in registers meanwhile.  The tile's comp[j], core_j and q_j are staged next to the operands (1.3
//                              KB).  Every thread keeps, for each of its four rows, the smallest (w, j) over its own j with comp[j] != comp[i]: its j
//                              ascend (v inside a tile, then the tiles) and the compare is strict, so among equal w the smallest j stays.  After the
//                              last tile the 16 threads that share a ty - 16 adjacent lanes of one wave - combine by four xor-shuffles under (w, j)
//                              ascending and lane tx = u < 4 stores row 4 ty + u.  For a fixed i, (w, j) ascending IS the edge order: j1 < j2 < i
//                              gives (j1, i) < (j2, i); i < j1 < j2 gives (i, j1) < (i, j2); j1 < i < j2 gives (j1, i) < (i, j2).  No LDS beyond the
//                              operand stages and the tile's 64 triples: the registers decide the residency.
//   mst_comp_w_kernel          thread = row: atomicMin(cw[comp[i]], the 64-bit pattern of the row's w) - the component's smallest weight
//   mst_comp_e_kernel          thread = row whose w IS cw[comp[i]]: atomicMin(ce[comp[i]], min(i, j) << 32 | max(i, j)) - among the rows that hold the
//                              smallest weight, the smallest (lo, hi): the component's smallest outgoing edge under the edge order
//   mst_hook_kernel            thread = root c: its edge reaches the root t.  Where t chose the same edge, the lower of c and t emits it and stays a
//                              root, the other hooks under it; every other root emits its edge and hooks under t.  parent[c] = t or c
//   mst_compress_kernel        thread = row: comp[i] = the fixed point of parent[parent[...comp[i]]], the walk cut at n steps (db_compress_kernel's manner)
// Why the hooks close no cycle.  Every root chose the smallest edge that leaves its component.  Take a cycle c1 -> c2 -> ... -> ck -> c1 of hooks, k >= 2,
// e_m the edge c_m chose.  e_m also leaves c_(m+1), so e_(m+1) <= e_m in the edge order; around the cycle every <= is an equality, and the order is
// strict: all k roots chose ONE edge.  An edge has two ends, so k = 2: the mutual case, which the rule above breaks by keeping the lower root.  There
// is no other cycle, the emitted edges are n - 1 distinct edges in all, and by the cut property each lies in the unique tree.
// Every root hooks or is the kept half of a mutual pair, so a round at least halves the component count: ceil(log2 n) rounds always suffice (the cap
// in ops.hip).  The host reads the edge count once per round (one stream wait each) and stops at n - 1.
//   mst_rank_kernel            thread = emitted edge: its rank = the number of emitted edges with a smaller key (w's pattern, lo << 32 | hi), the keys
//                              streamed through LDS 256 at a time; the keys are distinct, so the ranks are 0 .. n - 2 once each; the edge goes to
//                              eu / ev / ew [rank].  Bounded and deterministic whatever order the hooks' atomicAdd handed the slots out in.
#include "kernels.h"

namespace gr {

constexpr int MS_T = 64;                // rows of a tile, on both sides of the pair
constexpr int MS_DC = 16;               // columns per LDS stage: 2 x 8.4 KB of operands
constexpr int MS_LD = MS_T + 2;         // leading dimension of a staged column: 16-byte aligned groups of 4 rows, columns 4 banks apart
constexpr int MS_DMAX = 256;
constexpr unsigned long long MS_NONE = ~0ull;

__global__ void mst_begin_kernel(const float* __restrict__ x, long n, int d, int metric, double* __restrict__ qn, int* __restrict__ comp,
                                 int* __restrict__ parent, int* __restrict__ n_edges) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *n_edges = 0;
  if (i >= n) return;
  comp[i] = (int)i;
  parent[i] = (int)i;
  if (metric == 1) {
    double p = 0.0;
    for (int t = 0; t < d; ++t) { const double v = (double)x[i * d + t]; p = p + v * v; }
    qn[i] = sqrt(p);
  }
}

// silhouette.hip's staged layout (sl_swz, sl_operands, sl_pair), restated here as knn.hip and density.hip restate it, so that those files' objects
// stay what they were: entries 4 tx .. 4 tx + 3 of a staged column are one thread's, read as two 16-byte halves; the halves of the threads tx >= 8
// are swapped, so that the 16 threads of a read group cover all 64 banks once
__device__ __forceinline__ int ms_swz(int r) { return r ^ ((r >> 4) & 2); }
__device__ __forceinline__ void ms_operands(const double (*As)[MS_LD], const double (*Bs)[MS_LD], int t, int tx, int ty, double* a, double* b) {
  const int sw = (tx >> 2) & 2;
  const double2 a01 = *reinterpret_cast<const double2*>(&As[t][4 * ty]), a23 = *reinterpret_cast<const double2*>(&As[t][4 * ty + 2]);
  const double2 b01 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + sw]), b23 = *reinterpret_cast<const double2*>(&Bs[t][4 * tx + (sw ^ 2)]);
  a[0] = a01.x; a[1] = a01.y; a[2] = a23.x; a[3] = a23.y;
  b[0] = b01.x; b[1] = b01.y; b[2] = b23.x; b[3] = b23.y;
}
template <int METRIC> __device__ __forceinline__ void ms_pair(double (&acc)[4][4], const double* a, const double* b) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (METRIC == 0) { const double df = a[u] - b[v]; acc[u][v] = acc[u][v] + df * df; }
      else acc[u][v] = acc[u][v] + a[u] * b[v];
    }
}

template <int METRIC>
__global__ __launch_bounds__(256) void mst_pair_kernel(const float* __restrict__ x, long n, int d, const double* __restrict__ qn,
                                                        const double* __restrict__ core, long core_stride, const int* __restrict__ comp,
                                                        double* __restrict__ best_w, int* __restrict__ best_j) {
  __shared__ __attribute__((aligned(16))) double As[MS_DC][MS_LD], Bs[MS_DC][MS_LD];
  __shared__ double Ks[MS_T], Qs[MS_T];                                 // the tile's core_j and q_j ...
  __shared__ int Cs[MS_T];                                              // ... and comp[j]; -1 past the table
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;            // thread = rows 4 ty .. 4 ty + 3 x tile entries 4 tx .. 4 tx + 3
  const long i0 = (long)blockIdx.x * MS_T;
  // the loader's role: column lc of the chunk, rows lr + LP q of the tile - MS_DC consecutive lanes read MS_DC consecutive floats of a row
  constexpr int LP = 256 / MS_DC, LQ = MS_T / LP;
  const int lc = tid % MS_DC, lr = tid / MS_DC;

  double ci[4], qi[4], bw[4];
  int gi[4], bj[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long i = i0 + 4 * ty + u;
    const bool in = i < n;
    gi[u] = in ? comp[i] : -1;
    ci[u] = (in && core) ? core[i * core_stride] : 0.0;
    qi[u] = (METRIC == 1 && in) ? qn[i] : 0.0;
    bw[u] = __longlong_as_double(0x7ff0000000000000ll);                 // +inf: above every weight
    bj[u] = 0x7fffffff;                                                 // no row yet
  }

  for (long j0 = 0; j0 < n; j0 += MS_T) {
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
    // the tile's triples, one row per thread of the first wave; written below, once the tile before has been read
    int sc = -1;
    double sk = 0.0, sq = 0.0;
    if (tid < MS_T && j0 + tid < n) {
      const long j = j0 + tid;
      sc = comp[j];
      if (core) sk = core[j * core_stride];
      if (METRIC == 1) sq = qn[j];
    }
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int c0 = 0; c0 < d; c0 += MS_DC) {
      const int dc = min(MS_DC, d - c0);
      __syncthreads();                                                  // the stage before this one, and the tile before, have been read
#pragma unroll
      for (int q = 0; q < LQ; ++q) { As[lc][lr + LP * q] = (double)fa[q]; Bs[lc][ms_swz(lr + LP * q)] = (double)fb[q]; }
      if (c0 == 0 && tid < MS_T) { Cs[tid] = sc; Ks[tid] = sk; Qs[tid] = sq; }
      __syncthreads();
      if (c0 + MS_DC < d) fetch(c0 + MS_DC);
      for (int t = 0; t < dc; ++t) {
        double a[4], b[4];
        ms_operands(As, Bs, t, tx, ty, a, b);
        ms_pair<METRIC>(acc, a, b);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {                                       // ascending j
      const int jt = 4 * tx + v;
      const int gj = Cs[jt];
      const double cj = Ks[jt];
      const double qj = METRIC == 1 ? Qs[jt] : 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        double dist;
        if (METRIC == 0) dist = sqrt(acc[u][v]);
        else {
          const double den = qi[u] * qj;
          const double c = (qi[u] == 0.0 || qj == 0.0) ? 0.0 : acc[u][v] / den;
          const double e = 1.0 - c;
          dist = e > 0.0 ? e : 0.0;
        }
        double w = dist;
        if (ci[u] > w) w = ci[u];
        if (cj > w) w = cj;
        const bool take = gj >= 0 && gi[u] >= 0 && gj != gi[u] && w < bw[u];      // strict: among equal weights the lower j stays
        if (take) { bw[u] = w; bj[u] = (int)j0 + jt; }
      }
    }
  }
  // every lane of the workgroup is here: the smallest (w, j) over the 16 lanes that share a ty
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const double ow = __shfl_xor(bw[u], off, 64);
      const int oj = __shfl_xor(bj[u], off, 64);
      if (ow < bw[u] || (ow == bw[u] && oj < bj[u])) { bw[u] = ow; bj[u] = oj; }
    }
  const int su = tx & 3;
  const double mw = su == 0 ? bw[0] : su == 1 ? bw[1] : su == 2 ? bw[2] : bw[3];
  const int mj = su == 0 ? bj[0] : su == 1 ? bj[1] : su == 2 ? bj[2] : bj[3];
  const long is = i0 + 4 * ty + tx;                                     // the storing lane's row (tx < 4)
  if (tx < 4 && is < n) { best_w[is] = mw; best_j[is] = mj == 0x7fffffff ? -1 : mj; }
}

// ------------------------------------------------------------------ the components' smallest outgoing edges
__global__ void mst_comp_w_kernel(const double* __restrict__ best_w, const int* __restrict__ best_j, const int* __restrict__ comp, long n,
                                  unsigned long long* cw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || best_j[i] < 0) return;
  atomicMin(&cw[comp[i]], (unsigned long long)__double_as_longlong(best_w[i]));
}

__global__ void mst_comp_e_kernel(const double* __restrict__ best_w, const int* __restrict__ best_j, const int* __restrict__ comp, long n,
                                  const unsigned long long* __restrict__ cw, unsigned long long* ce) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = best_j[i];
  if (j < 0) return;
  const int g = comp[i];
  if ((unsigned long long)__double_as_longlong(best_w[i]) != cw[g]) return;
  const unsigned lo = (unsigned)min((int)i, j), hi = (unsigned)max((int)i, j);
  atomicMin(&ce[g], ((unsigned long long)lo << 32) | hi);
}

__global__ void mst_hook_kernel(const int* __restrict__ comp, long n, const unsigned long long* __restrict__ cw, const unsigned long long* __restrict__ ce,
                                int* __restrict__ parent, int* n_edges, unsigned long long* __restrict__ edge_w, unsigned long long* __restrict__ edge_e) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n || comp[c] != (int)c) return;                              // roots only
  const unsigned long long e = ce[c];
  if (e == MS_NONE) return;                                             // the one component that is left has no outgoing edge
  const long lo = (long)(e >> 32), hi = (long)(e & 0xffffffffull);
  if (lo >= n || hi >= n) return;                                       // (cannot be: the keys are rows of the table)
  const int t = comp[lo] == (int)c ? comp[hi] : comp[lo];
  const bool mutual = ce[t] == e;
  if (mutual && t < (int)c) { parent[c] = t; return; }                  // the lower root of the two emits the edge they share
  parent[c] = mutual ? (int)c : t;
  const int slot = atomicAdd(n_edges, 1);
  if (slot < n - 1) { edge_w[slot] = cw[c]; edge_e[slot] = e; }
}

__global__ void mst_compress_kernel(const int* __restrict__ parent, long n, int* __restrict__ comp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int r = comp[i];                                                      // parent is not written here, and comp[i] by this thread alone
  for (long step = 0; step < n; ++step) {                               // a forest: fewer than n steps
    const int up = parent[r];
    if (up == r) break;
    r = up;
  }
  comp[i] = r;
}

// ------------------------------------------------------------------ the emitted edges in the edge order
__global__ __launch_bounds__(256) void mst_rank_kernel(const unsigned long long* __restrict__ edge_w, const unsigned long long* __restrict__ edge_e, long m,
                                                        int* __restrict__ eu, int* __restrict__ ev, double* __restrict__ ew) {
  __shared__ unsigned long long Ws[256], Es[256];
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const bool mine = e < m;
  const unsigned long long kw = mine ? edge_w[e] : 0ull, ke = mine ? edge_e[e] : 0ull;
  long rank = 0;
  for (long f0 = 0; f0 < m; f0 += 256) {
    const long f = f0 + threadIdx.x;
    __syncthreads();
    Ws[threadIdx.x] = f < m ? edge_w[f] : MS_NONE;                      // past the end: above every key
    Es[threadIdx.x] = f < m ? edge_e[f] : MS_NONE;
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < 256; ++t) rank += (Ws[t] < kw || (Ws[t] == kw && Es[t] < ke)) ? 1 : 0;
  }
  if (mine && rank < m) {                                               // distinct keys: every rank once
    eu[rank] = (int)(ke >> 32);
    ev[rank] = (int)(ke & 0xffffffffull);
    ew[rank] = __longlong_as_double((long long)kw);
  }
}

// ------------------------------------------------------------------ launchers
// doubles: q [n], best_w [n]; words: cw [n], ce [n], edge_w [n], edge_e [n]; ints: comp [n], parent [n], best_j [n], n_edges [1]: 60 n bytes and change
static size_t ms_align(size_t bytes) { return (bytes + 255) / 256 * 256; }
size_t mst_workspace_bytes(long n) { return 6 * ms_align(8 * (size_t)n) + 3 * ms_align(sizeof(int) * (size_t)n) + ms_align(sizeof(int)); }

MstScratch mst_carve(void* workspace, long n) {
  char* ws = static_cast<char*>(workspace);
  auto take = [&](size_t bytes) { char* p = ws; ws += ms_align(bytes); return p; };
  MstScratch w;
  w.qn = reinterpret_cast<double*>(take(8 * (size_t)n));
  w.best_w = reinterpret_cast<double*>(take(8 * (size_t)n));
  w.cw = reinterpret_cast<unsigned long long*>(take(8 * (size_t)n));    // cw and ce lie next to each other: one memset resets both
  w.ce = reinterpret_cast<unsigned long long*>(take(8 * (size_t)n));
  w.edge_w = reinterpret_cast<unsigned long long*>(take(8 * (size_t)n));
  w.edge_e = reinterpret_cast<unsigned long long*>(take(8 * (size_t)n));
  w.comp = reinterpret_cast<int*>(take(sizeof(int) * (size_t)n));
  w.parent = reinterpret_cast<int*>(take(sizeof(int) * (size_t)n));
  w.best_j = reinterpret_cast<int*>(take(sizeof(int) * (size_t)n));
  w.n_edges = reinterpret_cast<int*>(take(sizeof(int)));
  return w;
}

int launch_mst_begin(const float* x, long n, int d, int metric, const MstScratch& w, hipStream_t s) {
  if (n < 2 || n > MST_MAX_N || d < 1 || d > MS_DMAX || (metric != 0 && metric != 1)) return 1;
  KtScope kt("mst_begin_kernel", metric ? 2.0 * n * d : 0.0, metric ? 4.0 * n * d : 8.0 * n, s);
  hipLaunchKernelGGL(mst_begin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, d, metric, w.qn, w.comp, w.parent, w.n_edges);
  return 0;
}

void launch_mst_round(const float* x, long n, int d, int metric, const double* core, long core_stride, const MstScratch& w, hipStream_t s) {
  const unsigned rows = (unsigned)((n + 255) / 256);
  {
    const unsigned grid = (unsigned)((n + MS_T - 1) / MS_T);
    KtScope kt(metric ? "mst_pair_kernel<cosine>" : "mst_pair_kernel<euclidean>", (metric ? 2.0 : 3.0) * n * n * d, 4.0 * n * d * grid, s);
    if (metric) hipLaunchKernelGGL(mst_pair_kernel<1>, dim3(grid), dim3(256), 0, s, x, n, d, w.qn, core, core_stride, w.comp, w.best_w, w.best_j);
    else hipLaunchKernelGGL(mst_pair_kernel<0>, dim3(grid), dim3(256), 0, s, x, n, d, w.qn, core, core_stride, w.comp, w.best_w, w.best_j);
  }
  KtScope kt("mst_component_kernels", 8.0 * n, 80.0 * n, s);
  (void)hipMemsetAsync(w.cw, 0xff, (size_t)(reinterpret_cast<char*>(w.ce) - reinterpret_cast<char*>(w.cw)) + 8 * (size_t)n, s);
  hipLaunchKernelGGL(mst_comp_w_kernel, dim3(rows), dim3(256), 0, s, w.best_w, w.best_j, w.comp, n, w.cw);
  hipLaunchKernelGGL(mst_comp_e_kernel, dim3(rows), dim3(256), 0, s, w.best_w, w.best_j, w.comp, n, w.cw, w.ce);
  hipLaunchKernelGGL(mst_hook_kernel, dim3(rows), dim3(256), 0, s, w.comp, n, w.cw, w.ce, w.parent, w.n_edges, w.edge_w, w.edge_e);
  hipLaunchKernelGGL(mst_compress_kernel, dim3(rows), dim3(256), 0, s, w.parent, n, w.comp);
}

void launch_mst_finish(long n, const MstScratch& w, int* eu, int* ev, double* ew, hipStream_t s) {
  const long m = n - 1;
  KtScope kt("mst_rank_kernel", 3.0 * m * m, 16.0 * m * ((m + 255) / 256), s);
  hipLaunchKernelGGL(mst_rank_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, w.edge_w, w.edge_e, m, eu, ev, ew);
}

}  // namespace gr
