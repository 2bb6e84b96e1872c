// kmeans.hip — clustering of the recovered noise vectors: apply_r.lua:197-243.
//
//   createClusterImages (apply_r.lua:197-231) = unsup.kmeans(attributes, nbClusters, nbIterations) followed by a
//   nearest-centroid pass in which the reference scores every (row, centroid) pair with cosineSimilarity (apply_r.lua:396-400)
//   and KEEPS THE MINIMUM (apply_r.lua:207-214: `dist < minDist`), i.e. the least similar centroid - preserved, flagged, and
//   selectable (take_min = 0 gives the most similar one).
//
// unsup.kmeans is an un-vendored luarock (koraykv/unsup, kmeans.lua; no version pinned by the reference).  Restated
// [upstream, from memory]: per iteration  c2 = 0.5 * sum(centroids^2, 2);  label(x) = argmax_j (centroid_j . x - c2_j)
// (first maximum wins);  centroid_j = sum of its rows / count (clusters that received no row keep their centroid);
// totalcounts += counts.  Upstream evaluates the products with sgemm and adds the member rows in fp32 (BLAS-defined order);
// here the dot products are sequential fp32 (j ascending, no FMA contraction: the oracle does the same, so labels are
// bit-reproducible) and the member sums are fp64, rounded to fp32 once before the fp32 division by the count.
// The initial centroids (upstream: k rows of N(0,1) from Torch's Mersenne twister, each divided by its norm) are an INPUT.
//
// Kernels (all HBM-bound: one pass over x[N][d] each):
//   kmeans_assign_kernel      thread = row, 256 rows x 32 columns staged through LDS per step, centroids via the scalar cache
//   kmeans_accumulate_kernel  workgroup = 512 consecutive rows, thread = column: fp64 sums per (cluster, column) in LDS, in row
//                             order (deterministic), one partial block per workgroup
//   kmeans_update_kernel      partial blocks summed in workgroup order; new centroids, c2, counts
//   cosine_assign_kernel      thread = row: the k cosine similarities in nn.CosineDistance's exact op order (fp32 products,
//                             fp64 sequential row sums, fp32 reciprocal / sqrt / multiply) and their arg-min or arg-max
//   cluster_members_*_kernel  apply_r.lua:218-227: per cluster the m most similar member rows, by a sort of (similarity, row) keys
//   cluster_faces_kernel      apply_r.lua:233-243: every cluster's average face in one launch
#include "kernels.h"

namespace gr {

constexpr int KM_ROWS = 256, KM_DC = 32, KM_KMAX = 32, KM_RPB = 512;

__global__ __launch_bounds__(KM_ROWS) void kmeans_assign_kernel(const float* __restrict__ x, long N, int d, const float* __restrict__ cent,
                                                                 const float* __restrict__ c2, int k, int* __restrict__ labels) {
  __shared__ __attribute__((aligned(16))) float tile[KM_ROWS * (KM_DC + 1)];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * KM_ROWS;
  float s[KM_KMAX];
#pragma unroll
  for (int j = 0; j < KM_KMAX; ++j) s[j] = 0.f;
  for (int c0 = 0; c0 < d; c0 += KM_DC) {
    const int dc = min(KM_DC, d - c0);
    for (int e = tid; e < KM_ROWS * KM_DC; e += KM_ROWS) {
      const int r = e / KM_DC, c = e - r * KM_DC;
      tile[r * (KM_DC + 1) + c] = (r0 + r < N && c < dc) ? x[(r0 + r) * (long)d + c0 + c] : 0.f;
    }
    __syncthreads();
    const float* row = tile + tid * (KM_DC + 1);
    for (int c = 0; c < dc; ++c) {
      const float b = row[c];
#pragma unroll
      for (int j = 0; j < KM_KMAX; ++j)
        if (j < k) s[j] = s[j] + cent[(long)j * d + c0 + c] * b;      // wave-uniform centroid address; no contraction (Makefile)
    }
    __syncthreads();
  }
  if (r0 + tid < N) {
    float best = 0.f; int bi = 0;
#pragma unroll
    for (int j = 0; j < KM_KMAX; ++j)
      if (j < k) { const float v = s[j] - c2[j]; if (j == 0 || v > best) { best = v; bi = j; } }
    labels[r0 + tid] = bi;
  }
}

__global__ __launch_bounds__(256) void kmeans_accumulate_kernel(const float* __restrict__ x, long N, int d, const int* __restrict__ labels, int k,
                                                                 double* __restrict__ part_sum /*[nblk][k][d]*/, int* __restrict__ part_cnt /*[nblk][k]*/) {
  extern __shared__ double acc[];                      // [k][d]
  __shared__ int lab[KM_RPB];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * KM_RPB;
  const int nr = (int)min((long)KM_RPB, N - r0);
  for (int e = tid; e < k * d; e += 256) acc[e] = 0.0;
  for (int e = tid; e < nr; e += 256) lab[e] = labels[r0 + e];
  __syncthreads();
  for (int t = tid; t < d; t += 256)                   // thread owns column t: adds the rows in order
    for (int r = 0; r < nr; ++r) acc[lab[r] * d + t] += (double)x[(r0 + r) * (long)d + t];
  if (tid < k) { int cnt = 0; for (int r = 0; r < nr; ++r) cnt += lab[r] == tid; part_cnt[(long)blockIdx.x * k + tid] = cnt; }
  __syncthreads();
  for (int e = tid; e < k * d; e += 256) part_sum[(long)blockIdx.x * k * d + e] = acc[e];
}

// one workgroup per cluster: sums the partial blocks in order, writes the new centroid row, its c2 and the counts
__global__ __launch_bounds__(256) void kmeans_update_kernel(const double* __restrict__ part_sum, const int* __restrict__ part_cnt, int nblk, int k, int d,
                                                             float* __restrict__ cent, float* __restrict__ c2, float* __restrict__ counts, float* __restrict__ totalcounts) {
  __shared__ double red[256];
  __shared__ int s_cnt;
  const int j = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) { int c = 0; for (int b = 0; b < nblk; ++b) c += part_cnt[(long)b * k + j]; s_cnt = c; }
  __syncthreads();
  const int cnt = s_cnt;
  double sq = 0.0;                                     // this thread's share of sum(centroid^2) (accreal = double, fixed order below)
  for (int t = tid; t < d; t += 256) {
    float v = cent[(long)j * d + t];
    if (cnt != 0) {
      double sm = 0.0;
      for (int b = 0; b < nblk; ++b) sm += part_sum[((long)b * k + j) * d + t];
      v = (float)sm / (float)cnt;                      // summation[i]:div(counts[i]) on float tensors
      cent[(long)j * d + t] = v;
    }
    const float p = v * v;                             // pow(centroids, 2) is a float tensor
    sq += (double)p;
  }
  red[tid] = sq;
  __syncthreads();
  if (tid == 0) {
    // torch.sum over the row: sequential in column order.  Thread t holds columns t, t+256, ...: for d <= 256 (every case of
    // the reference: d = noise dimension) summing red[] in thread order IS column order.
    double tot = 0.0;
    for (int t = 0; t < 256; ++t) tot += red[t];
    c2[j] = (float)tot * 0.5f;
    counts[j] = (float)cnt;
    totalcounts[j] += (float)cnt;
  }
}

__global__ void kmeans_c2_kernel(const float* __restrict__ cent, int k, int d, float* __restrict__ c2) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  double s = 0.0;
  for (int t = 0; t < d; ++t) { const float p = cent[(long)j * d + t] * cent[(long)j * d + t]; s += (double)p; }
  c2[j] = (float)s * 0.5f;
}

// w32[j] = 1 / (sum(c_j^2) + 1e-12) in nn.CosineDistance's op order
__global__ void cosine_centroid_prep_kernel(const float* __restrict__ cent, int k, int d, float* __restrict__ w32) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  double s = 0.0;
  for (int t = 0; t < d; ++t) { const float p = cent[(long)j * d + t] * cent[(long)j * d + t]; s += (double)p; }
  float w = (float)s;
  w = w + 1e-12f;
  w32[j] = 1.f / w;
}

__global__ __launch_bounds__(KM_ROWS) void cosine_assign_kernel(const float* __restrict__ x, long N, int d, const float* __restrict__ cent,
                                                                 const float* __restrict__ w32, int k, int take_min,
                                                                 int* __restrict__ labels, float* __restrict__ sims) {
  __shared__ __attribute__((aligned(16))) float tile[KM_ROWS * (KM_DC + 1)];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * KM_ROWS;
  float best = 0.f; int bi = 0;
  for (int j0 = 0; j0 < k; j0 += KM_KMAX) {            // KM_KMAX centroids per pass over the row (one pass for k <= 32)
    const int kk = min(KM_KMAX, k - j0);
    double s1[KM_KMAX], s2 = 0.0;
#pragma unroll
    for (int j = 0; j < KM_KMAX; ++j) s1[j] = 0.0;
    for (int c0 = 0; c0 < d; c0 += KM_DC) {
      const int dc = min(KM_DC, d - c0);
      for (int e = tid; e < KM_ROWS * KM_DC; e += KM_ROWS) {
        const int r = e / KM_DC, c = e - r * KM_DC;
        tile[r * (KM_DC + 1) + c] = (r0 + r < N && c < dc) ? x[(r0 + r) * (long)d + c0 + c] : 0.f;
      }
      __syncthreads();
      const float* row = tile + tid * (KM_DC + 1);
      for (int c = 0; c < dc; ++c) {
        const float a = row[c];
        const float aa = a * a;
        s2 += (double)aa;
#pragma unroll
        for (int j = 0; j < KM_KMAX; ++j)
          if (j < kk) { const float p = a * cent[(long)(j0 + j) * d + c0 + c]; s1[j] += (double)p; }
      }
      __syncthreads();
    }
    float w22 = (float)s2;
    w22 = w22 + 1e-12f; w22 = 1.f / w22;
#pragma unroll
    for (int j = 0; j < KM_KMAX; ++j)
      if (j < kk) {
        float w = w22 * w32[j0 + j];
        w = sqrtf(w);
        const float sc = (float)s1[j] * w;
        const bool first = j0 + j == 0;
        if (first || (take_min ? sc < best : sc > best)) { best = sc; bi = j0 + j; }
      }
  }
  if (r0 + tid < N) { labels[r0 + tid] = bi; sims[r0 + tid] = best; }
}

size_t kmeans_workspace_bytes(long N, int d, int k) {
  const long nblk = (N + KM_RPB - 1) / KM_RPB;
  return sizeof(double) * (size_t)nblk * k * d + sizeof(int) * (size_t)nblk * k + sizeof(int) * (size_t)N + 1024;
}

// x, cent (in: initial, out: final), c2 / counts / totalcounts [k] are device buffers; workspace from kmeans_workspace_bytes
int launch_kmeans(const float* x, long N, int d, int k, int niter, float* cent, float* c2, float* counts, float* totalcounts,
                  int* labels_out /*nullable: labels of the last iteration*/, void* workspace, hipStream_t s) {
  if (k > KM_KMAX || (size_t)k * d * sizeof(double) > 60 * 1024 || d > 256) return 1;
  const long nblk = (N + KM_RPB - 1) / KM_RPB;
  double* part_sum = reinterpret_cast<double*>(workspace);
  int* part_cnt = reinterpret_cast<int*>(part_sum + (size_t)nblk * k * d);
  int* labels = labels_out ? labels_out : part_cnt + (size_t)nblk * k;
  (void)hipMemsetAsync(totalcounts, 0, sizeof(float) * k, s);
  hipLaunchKernelGGL(kmeans_c2_kernel, dim3(1), dim3(64), 0, s, cent, k, d, c2);
  const size_t lds = sizeof(double) * (size_t)k * d;
  for (int it = 0; it < niter; ++it) {
    { KtScope kt("kmeans_assign_kernel", 2.0 * N * d * k, 4.0 * N * d, s);
      hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)((N + KM_ROWS - 1) / KM_ROWS)), dim3(KM_ROWS), 0, s, x, N, d, cent, c2, k, labels); }
    { KtScope kt("kmeans_accumulate_kernel", (double)N * d, 4.0 * N * d, s);
      hipLaunchKernelGGL(kmeans_accumulate_kernel, dim3((unsigned)nblk), dim3(256), lds, s, x, N, d, labels, k, part_sum, part_cnt); }
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(k), dim3(256), 0, s, part_sum, part_cnt, (int)nblk, k, d, cent, c2, counts, totalcounts);
  }
  return 0;
}

int launch_cosine_assign(const float* x, long N, int d, const float* cent, int k, int take_min, float* w32 /*[k] scratch*/,
                         int* labels, float* sims, hipStream_t s) {
  if (k <= 0) return 1;
  hipLaunchKernelGGL(cosine_centroid_prep_kernel, dim3((k + 63) / 64), dim3(64), 0, s, cent, k, d, w32);
  KtScope kt("cosine_assign_kernel", 2.0 * N * d * k, 4.0 * N * d, s);
  hipLaunchKernelGGL(cosine_assign_kernel, dim3((unsigned)((N + KM_ROWS - 1) / KM_ROWS)), dim3(KM_ROWS), 0, s, x, N, d, cent, w32, k, take_min, labels, sims);
  return 0;
}

// ------------------------------------------------------------------ apply_r.lua:218-227: the nbMaxPerCluster most similar rows of each cluster
// table.sort(cluster, a[2] > b[2]) and the first m entries, as numpy's stable argsort of -similarity orders them: similarity descending (-0 and
// +0 are one value), ties by ascending row, NaN after every number.  Every member row gets a 64-bit key, (order-preserving image of
// -similarity) << 32 | row: keys are distinct, so "the m smallest keys, ascending" is one well-defined list and nothing depends on the order in
// which threads meet the rows.  cluster_members_partial_kernel: workgroup = (cluster, one of S contiguous row ranges); it keeps the range's m
// smallest keys in LDS (candidates below the current m-th key are appended by a block prefix sum, the 512-key buffer is sorted and cut to m
// when it runs full).  cluster_members_merge_kernel: workgroup = cluster, sorts the S lists and writes the result.
constexpr int CM_MMAX = 128, CM_U = 16, CM_BUF = 512, CM_SMAX = 8;
constexpr unsigned long long CM_NONE = ~0ull;

__device__ inline unsigned long long cm_key(float sim, long row) {
  unsigned u = 0xFFFFFFFFu;                                             // NaN: after every number
  if (sim == sim) {
    const float f = sim == 0.f ? 0.f : -sim;
    u = __float_as_uint(f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                     // unsigned order = order of f
  }
  return ((unsigned long long)u << 32) | (unsigned long long)row;
}
// ascending bitonic sort of buf[0, P) by 256 threads (P a power of two, >= 512); ends with a barrier
template <int P> __device__ __noinline__ void cm_sort(unsigned long long* buf, int tid) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < P / 2; i += 256) {
        const int a = 2 * i - (i & (stride - 1)), b = a + stride;
        const unsigned long long ka = buf[a], kb = buf[b];
        if ((ka > kb) == ((a & size) == 0)) { buf[a] = kb; buf[b] = ka; }
      }
    }
  __syncthreads();
}

__global__ __launch_bounds__(256) void cluster_members_partial_kernel(const int* __restrict__ labels, const float* __restrict__ sims, long n, int m, int S,
                                                                       unsigned long long* __restrict__ part_keys /*[k][S][CM_MMAX]*/, int* __restrict__ part_cnt /*[k][S]*/) {
  __shared__ unsigned long long buf[CM_BUF];
  __shared__ int wsum[2][4];
  __shared__ int s_members;
  const int j = blockIdx.x, sp = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long chunk = 256L * CM_U;
  const long per = ((n + S - 1) / S + chunk - 1) / chunk * chunk;
  const long lo = sp * per, hi = min(n, lo + per);
  buf[tid] = CM_NONE; buf[tid + 256] = CM_NONE;
  if (tid == 0) s_members = 0;
  int count = 0, members = 0, par = 0;                                  // count: keys in buf (the same number in every thread)
  unsigned long long thr = CM_NONE;                                     // a key must be below it to matter: the m-th smallest so far, once m are known
  __syncthreads();
  for (long base = lo; base < hi; base += chunk) {
    unsigned long long key[CM_U];
    bool any = false;
#pragma unroll
    for (int u = 0; u < CM_U; ++u) {
      const long row = base + u * 256 + tid;
      key[u] = CM_NONE;
      if (row < hi && labels[row] == j) {
        ++members;
        const unsigned long long kk = cm_key(sims[row], row);
        if (kk < thr) { key[u] = kk; any = true; }
      }
    }
    if (!__syncthreads_or(any)) continue;
#pragma unroll
    for (int u = 0; u < CM_U; ++u) {
      const bool f = key[u] < thr;                                      // (CM_NONE is below nothing)
      const unsigned long long bal = __ballot(f);
      if (lane == 0) wsum[par][w] = __popcll(bal);
      __syncthreads();
      int off = 0, tot = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) { const int v = wsum[par][q]; if (q < w) off += v; tot += v; }
      par ^= 1;
      if (f) buf[count + off + __popcll(bal & ((1ull << lane) - 1ull))] = key[u];
      count += tot;
      if (count > CM_BUF - 256) {                                       // the next 256 rows might not fit: sort, keep the m smallest
        cm_sort<CM_BUF>(buf, tid);
        count = min(count, m);
        if (tid >= count) buf[tid] = CM_NONE;
        buf[tid + 256] = CM_NONE;
        __syncthreads();
        if (count == m) thr = buf[m - 1];
      }
    }
  }
  cm_sort<CM_BUF>(buf, tid);
  if (members) atomicAdd(&s_members, members);                          // an integer sum: the same in any order
  __syncthreads();
  if (tid < CM_MMAX) part_keys[((long)j * S + sp) * CM_MMAX + tid] = tid < min(count, m) ? buf[tid] : CM_NONE;
  if (tid == 0) part_cnt[j * S + sp] = s_members;
}

__global__ __launch_bounds__(256) void cluster_members_merge_kernel(const unsigned long long* __restrict__ part_keys, const int* __restrict__ part_cnt, int S, int m,
                                                                     const float* __restrict__ sims, long* __restrict__ rows_out, float* __restrict__ sims_out,
                                                                     int* __restrict__ kept_out, int* __restrict__ sizes_out) {
  __shared__ unsigned long long buf[CM_SMAX * CM_MMAX];
  const int j = blockIdx.x, tid = threadIdx.x;
  for (int e = tid; e < CM_SMAX * CM_MMAX; e += 256) buf[e] = e < S * CM_MMAX ? part_keys[(long)j * S * CM_MMAX + e] : CM_NONE;
  cm_sort<CM_SMAX * CM_MMAX>(buf, tid);
  int size = 0;
  for (int q = 0; q < S; ++q) size += part_cnt[j * S + q];
  const int kept = min(size, m);
  for (int e = tid; e < m; e += 256) {
    const long row = e < kept ? (long)(buf[e] & 0xFFFFFFFFull) : -1;
    rows_out[(long)j * m + e] = row;
    sims_out[(long)j * m + e] = e < kept ? sims[row] : 0.f;
  }
  if (tid == 0) { kept_out[j] = kept; sizes_out[j] = size; }
}

static int cluster_members_splits(long n) { return (int)min((long)CM_SMAX, max(1L, n / 65536)); }
size_t cluster_members_workspace_bytes(long n, int k) {
  return (sizeof(unsigned long long) * CM_MMAX + sizeof(int)) * (size_t)k * cluster_members_splits(n) + 256;
}
int launch_cluster_members(const int* labels, const float* sims, long n, int k, int m, long* rows_out, float* sims_out, int* kept_out, int* sizes_out,
                           void* workspace, hipStream_t s) {
  if (k < 1 || k > KM_KMAX || m < 1 || m > CM_MMAX || n < 1 || n > 0x7FFFFFFFL) return 1;
  const int S = cluster_members_splits(n);
  unsigned long long* part_keys = reinterpret_cast<unsigned long long*>(workspace);
  int* part_cnt = reinterpret_cast<int*>(part_keys + (size_t)k * S * CM_MMAX);
  { KtScope kt("cluster_members_partial_kernel", (double)n * k, 8.0 * n * k, s);
    hipLaunchKernelGGL(cluster_members_partial_kernel, dim3(k, S), dim3(256), 0, s, labels, sims, n, m, S, part_keys, part_cnt); }
  KtScope kt("cluster_members_merge_kernel", 0.0, 8.0 * k * S * CM_MMAX, s);
  hipLaunchKernelGGL(cluster_members_merge_kernel, dim3(k), dim3(256), 0, s, part_keys, part_cnt, S, m, sims, rows_out, sims_out, kept_out, sizes_out);
  return 0;
}

// ------------------------------------------------------------------ apply_r.lua:233-243: the average faces of all clusters
// Per cluster rows_mean_kernel's arithmetic (render.hip): the listed rows added in list order in fp32, one division by the list's length.  The
// lists are device data nobody has looked at: an entry outside [0, n_rows) is skipped (the divisor stays kept[j]).
__global__ __launch_bounds__(256) void cluster_faces_kernel(const float* __restrict__ x, long n_rows, long d, const long* __restrict__ rows /*[k][m]*/,
                                                             const int* __restrict__ kept, int m, float* __restrict__ out /*[k][d]*/) {
  const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const int j = blockIdx.y;
  if (p >= d) return;
  const int n = min(max(kept[j], 0), m);
  float acc = 0.f;
  for (int i = 0; i < n; ++i) {
    const long r = rows[(long)j * m + i];
    if (r >= 0 && r < n_rows) acc = acc + x[r * d + p];
  }
  out[(long)j * d + p] = n > 0 ? acc / (float)n : 0.f;
}
void launch_cluster_faces(const float* x, long n_rows, long d, const long* rows, const int* kept, int k, int m, float* out, hipStream_t s) {
  KtScope kt("cluster_faces_kernel", (double)k * m * (double)d, 4.0 * ((double)k * m + k) * (double)d, s);
  hipLaunchKernelGGL(cluster_faces_kernel, dim3((unsigned)((d + 255) / 256), k), dim3(256), 0, s, x, n_rows, d, rows, kept, m, out);
}

}  // namespace gr
