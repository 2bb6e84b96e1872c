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
//   kmeans_accumulate_kernel  workgroup = ROWS_PER_BLOCK consecutive rows, thread = column: fp64 sums per (cluster, column) in LDS, in row
//                             order (deterministic), one partial block per workgroup
//   kmeans_update_kernel      partial blocks summed in workgroup order; new centroids, c2, counts
//   cosine_assign_kernel      thread = row: the k cosine similarities in nn.CosineDistance's exact op order (fp32 products,
//                             fp64 sequential row sums, fp32 reciprocal / sqrt / multiply) and their arg-min or arg-max
//   cluster_members_*_kernel  apply_r.lua:218-227: per cluster the m most similar member rows, by a sort of (similarity, row) keys
//   cluster_faces_kernel      apply_r.lua:233-243: every cluster's average face in one launch
//   *_wide_kernel             gr_cluster_dev above 32 clusters: the same arithmetic, bit for bit, for k <= 4096 (listed where they start)
#include "kernels.h"

namespace gr {

constexpr int KM_ROWS = 256, KM_DC = 32, KM_KMAX = 32;

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
  __shared__ int lab[ROWS_PER_BLOCK];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * ROWS_PER_BLOCK;
  const int nr = (int)min((long)ROWS_PER_BLOCK, N - r0);
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
  const long nblk = row_blocks(N);
  return sizeof(double) * (size_t)nblk * k * d + sizeof(int) * (size_t)nblk * k + sizeof(int) * (size_t)N + 1024;
}

// x, cent (in: initial, out: final), c2 / counts / totalcounts [k] are device buffers; workspace from kmeans_workspace_bytes
int launch_kmeans(const float* x, long N, int d, int k, int niter, float* cent, float* c2, float* counts, float* totalcounts,
                  int* labels_out /*nullable: labels of the last iteration*/, void* workspace, hipStream_t s) {
  if (k > KM_KMAX || (size_t)k * d * sizeof(double) > 60 * 1024 || d > 256) return 1;
  const long nblk = row_blocks(N);
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

// ------------------------------------------------------------------ gr_cluster_dev: the whole of apply_r.lua:198-227, any k <= 4096
// Narrow route (k < g_cluster_wide_min_k and k * d doubles within the accumulate kernel's 60 KB of LDS): launch_kmeans, launch_cosine_assign,
// launch_cluster_members as they stand.  Wide route: the kernels below, which reproduce the narrow ones' bits for every k both take -
//   kmeans_assign_wide_kernel  workgroup = 128 rows held in LDS for the whole call (stage_rows, kernels.h), centroid tiles of KW_KT = 128 visited in ascending j and staged
//                              32 columns at a time; thread = 4 rows x 16 centroids (a half-wave shares its 16 centroids, its 32 lanes hold the
//                              rows: about 8 (rows + centroids) LDS cycles against 2 rows x centroids VALU cycles per column and CU; 2 x 16 measured
//                              2.2x the unfused VALU floor at k = 4096, 4 x 16 1.9x: DESIGN section 4), every (row, centroid) pair one sequential fp32 chain in column
//                              order (rounded multiply, rounded add).  The first maximum over j is "largest value, lowest index among equals, label 0
//                              when score 0 is a NaN", which is what the sequential strict > scan yields and does not depend on the visiting order
//   wide_group_kernel          stable grouping of a 512-row block by label (cm_sort of (label, row) keys): the block's rows in (label, row) order
//                              and the list of its (label, first position) segments - an index of O(n) entries, whatever k
//   wide_segment_sum_kernel    one fp64 partial per (cluster, block) segment and column, rows added in row order from +0.0
//   kmeans_update_wide_kernel  workgroup = cluster: finds its segment in every block (binary search of the block's sorted label list, 256 blocks
//                              at a time, hits kept in block order), adds the partials in block order from +0.0, then kmeans_update_kernel's tail
//   cosine_assign_wide_kernel  the same shape with cosine_assign_kernel's arithmetic (fp32 products, sequential fp64 sums)
//   cluster_members_wide_kernel  workgroup = cluster: walks its segments of the index grouped by the cosine labels and keeps the m smallest
//                              cm_key keys as cluster_members_partial_kernel does (a set of distinct keys, sorted: independent of the visiting order)
int g_cluster_wide_min_k = 33;          // gr_set_tuning "cluster_wide_min_k": the wide route from this k on (tests set 1 to compare the routes)
constexpr int KW_TR = 128, KW_RT = 4, KW_KT = 128, KW_DC = 32, KW_CLD = 132, KW_KMAX = 4096, KW_SEGMAX = ROWS_PER_BLOCK;   // rows: 32 lanes x KW_RT; centroids of a tile: 4 waves x 2 half-waves x 16

__global__ __launch_bounds__(256) void kmeans_assign_wide_kernel(const float* __restrict__ x, long N, int d, const float* __restrict__ cent,
                                                                  const float* __restrict__ c2, int k, int* __restrict__ labels) {
  extern __shared__ __attribute__((aligned(16))) float xs[];            // [KW_TR][ld], ld odd: lanes of a wave read distinct banks
  __shared__ __attribute__((aligned(16))) float cs[KW_DC * KW_CLD];     // [column of the chunk][centroid of the tile]
  __shared__ float cb[8 * KW_TR];
  __shared__ int ci[8 * KW_TR];
  __shared__ int nan0[KW_TR];
  const int tid = threadIdx.x, w = tid >> 6, rl = tid & 31, hw = tid >> 5;   // rows rl + 32 q; half-wave hw = centroids hw * 16 .. + 16 of the tile
  const int ld = d | 1;
  const long r0 = (long)blockIdx.x * KW_TR;
  const int nr = (int)min((long)KW_TR, N - r0);
  stage_rows<KW_TR>(x, r0, nr, d, ld, xs, tid);
  float best[KW_RT];
  int bi[KW_RT];
  bool first_nan[KW_RT];
#pragma unroll
  for (int q = 0; q < KW_RT; ++q) { best[q] = -INFINITY; bi[q] = -1; first_nan[q] = false; }
  for (int j0 = 0; j0 < k; j0 += KW_KT) {
    float acc[KW_RT][16];
#pragma unroll
    for (int q = 0; q < KW_RT; ++q)
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) acc[q][jj] = 0.f;
    for (int c0 = 0; c0 < d; c0 += KW_DC) {
      const int dc = min(KW_DC, d - c0);
      __syncthreads();                                                  // the chunk before this one has been read (and xs is written)
      for (int e = tid; e < KW_DC * KW_KT; e += 256) {
        const int jj = e / KW_DC, cc = e - jj * KW_DC;
        cs[cc * KW_CLD + jj] = (j0 + jj < k && cc < dc) ? cent[(long)(j0 + jj) * d + c0 + cc] : 0.f;
      }
      __syncthreads();
      if (j0 + w * 32 < k)                                              // (wave-uniform; a half-wave past k multiplies the tile's zero padding)
        for (int c = 0; c < dc; ++c) {
          float xv[KW_RT];
#pragma unroll
          for (int q = 0; q < KW_RT; ++q) xv[q] = xs[(rl + 32 * q) * ld + c0 + c];
          const float4* cp = reinterpret_cast<const float4*>(cs + c * KW_CLD + hw * 16);
          float cv[16];
#pragma unroll
          for (int g = 0; g < 4; ++g) { const float4 v = cp[g]; cv[4 * g] = v.x; cv[4 * g + 1] = v.y; cv[4 * g + 2] = v.z; cv[4 * g + 3] = v.w; }
#pragma unroll
          for (int q = 0; q < KW_RT; ++q)
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) acc[q][jj] = acc[q][jj] + cv[jj] * xv[q];      // no contraction (Makefile): kmeans_assign_kernel's chain
        }
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = j0 + hw * 16 + jj;
      if (j < k) {
        const float cc2 = c2[j];
#pragma unroll
        for (int q = 0; q < KW_RT; ++q) {
          const float v = acc[q][jj] - cc2;
          if (j == 0 && v != v) first_nan[q] = true;
          if (v > best[q]) { best[q] = v; bi[q] = j; }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KW_RT; ++q) {
    cb[hw * KW_TR + rl + 32 * q] = best[q];
    ci[hw * KW_TR + rl + 32 * q] = bi[q];
    if (hw == 0) nan0[rl + 32 * q] = first_nan[q];
  }
  __syncthreads();
  if (tid < nr) {
    float b = -INFINITY; int idx = -1;
    for (int q = 0; q < 8; ++q) {                                       // half-waves hold interleaved index ranges: largest value, lowest index among equals
      const float v = cb[q * KW_TR + tid]; const int i = ci[q * KW_TR + tid];
      if (i >= 0 && (idx < 0 || v > b || (v == b && i < idx))) { b = v; idx = i; }
    }
    labels[r0 + tid] = (idx < 0 || nan0[tid]) ? 0 : idx;
  }
}

// cosine_assign_kernel's arithmetic in kmeans_assign_wide_kernel's shape: per (row, centroid) the fp32 products a * c added one by one in fp64 in
// column order, the row's own sum of squares likewise, then fp32 reciprocal, multiply, square root and multiply.  The sequential scan `first or
// sc < best` (take_min; `>` otherwise) yields the smallest (largest) value, the lowest index among equals, and centroid 0 with its score when
// that score is a NaN or nothing beats it: which is what the waves' running results are merged to.
__global__ __launch_bounds__(256) void cosine_assign_wide_kernel(const float* __restrict__ x, long N, int d, const float* __restrict__ cent,
                                                                  const float* __restrict__ w32, int k, int take_min,
                                                                  int* __restrict__ labels, float* __restrict__ sims) {
  extern __shared__ __attribute__((aligned(16))) float xs[];            // [KW_TR][ld]
  __shared__ __attribute__((aligned(16))) float cs[KW_DC * KW_CLD];
  __shared__ float cb[8 * KW_TR];
  __shared__ int ci[8 * KW_TR];
  __shared__ float sc0[KW_TR];
  const int tid = threadIdx.x, w = tid >> 6, rl = tid & 31, hw = tid >> 5;   // rows rl + 32 q; half-wave hw = centroids hw * 16 .. + 16 of the tile
  const int ld = d | 1;
  const long r0 = (long)blockIdx.x * KW_TR;
  const int nr = (int)min((long)KW_TR, N - r0);
  stage_rows<KW_TR>(x, r0, nr, d, ld, xs, tid);
  const float none = take_min ? INFINITY : -INFINITY;
  float best[KW_RT];
  int bi[KW_RT];
  double s2[KW_RT];
#pragma unroll
  for (int q = 0; q < KW_RT; ++q) { best[q] = none; bi[q] = -1; s2[q] = 0.0; }
  for (int j0 = 0; j0 < k; j0 += KW_KT) {
    double acc[KW_RT][16];
#pragma unroll
    for (int q = 0; q < KW_RT; ++q)
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) acc[q][jj] = 0.0;
    for (int c0 = 0; c0 < d; c0 += KW_DC) {
      const int dc = min(KW_DC, d - c0);
      __syncthreads();
      for (int e = tid; e < KW_DC * KW_KT; e += 256) {
        const int jj = e / KW_DC, cc = e - jj * KW_DC;
        cs[cc * KW_CLD + jj] = (j0 + jj < k && cc < dc) ? cent[(long)(j0 + jj) * d + c0 + cc] : 0.f;
      }
      __syncthreads();
      if (j0 + w * 32 < k)                                              // (wave-uniform)
        for (int c = 0; c < dc; ++c) {
          float xv[KW_RT];
#pragma unroll
          for (int q = 0; q < KW_RT; ++q) xv[q] = xs[(rl + 32 * q) * ld + c0 + c];
          if (j0 == 0) {                                                // the row's own norm, once
#pragma unroll
            for (int q = 0; q < KW_RT; ++q) { const float a = xv[q] * xv[q]; s2[q] += (double)a; }
          }
          const float4* cp = reinterpret_cast<const float4*>(cs + c * KW_CLD + hw * 16);
          float cv[16];
#pragma unroll
          for (int g = 0; g < 4; ++g) { const float4 v = cp[g]; cv[4 * g] = v.x; cv[4 * g + 1] = v.y; cv[4 * g + 2] = v.z; cv[4 * g + 3] = v.w; }
#pragma unroll
          for (int q = 0; q < KW_RT; ++q)
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) { const float p = xv[q] * cv[jj]; acc[q][jj] += (double)p; }
        }
    }
#pragma unroll
    for (int q = 0; q < KW_RT; ++q) {
      float w22 = (float)s2[q];
      w22 = w22 + 1e-12f; w22 = 1.f / w22;
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = j0 + hw * 16 + jj;
        if (j < k) {
          float ww = w22 * w32[j];
          ww = sqrtf(ww);
          const float sc = (float)acc[q][jj] * ww;
          if (j == 0) sc0[rl + 32 * q] = sc;
          if (take_min ? sc < best[q] : sc > best[q]) { best[q] = sc; bi[q] = j; }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KW_RT; ++q) {
    cb[hw * KW_TR + rl + 32 * q] = best[q];
    ci[hw * KW_TR + rl + 32 * q] = bi[q];
  }
  __syncthreads();
  if (tid < nr) {
    float b = none; int idx = -1;
    for (int q = 0; q < 8; ++q) {
      const float v = cb[q * KW_TR + tid]; const int i = ci[q * KW_TR + tid];
      if (i >= 0 && (idx < 0 || (take_min ? v < b : v > b) || (v == b && i < idx))) { b = v; idx = i; }
    }
    const float first = sc0[tid];
    const bool keep0 = idx < 0 || first != first;
    labels[r0 + tid] = keep0 ? 0 : idx;
    sims[r0 + tid] = keep0 ? first : b;
  }
}

// labels of one 512-row block -> the block's rows in (label, row) order, and its segments: seg_label / seg_start [block][segs] (ascending labels,
// first position in the block's order), nseg [block], nvalid [block] = rows with a label in [0, k)
__global__ __launch_bounds__(256) void wide_group_kernel(const int* __restrict__ labels, long N, int k, int segs, int* __restrict__ order,
                                                          int* __restrict__ seg_label, int* __restrict__ seg_start, int* __restrict__ nseg, int* __restrict__ nvalid) {
  __shared__ unsigned long long buf[ROWS_PER_BLOCK];
  __shared__ int scan[2][ROWS_PER_BLOCK];
  const int tid = threadIdx.x, b = blockIdx.x;
  const long r0 = (long)b * ROWS_PER_BLOCK;
  const int nr = (int)min((long)ROWS_PER_BLOCK, N - r0);
  for (int i = tid; i < ROWS_PER_BLOCK; i += 256) {
    const int lab = i < nr ? labels[r0 + i] : -1;
    buf[i] = (lab >= 0 && lab < k) ? ((unsigned long long)lab << 32) | (unsigned)i : CM_NONE;
  }
  cm_sort<ROWS_PER_BLOCK>(buf, tid);
  for (int i = tid; i < ROWS_PER_BLOCK; i += 256) {
    const unsigned long long key = buf[i];
    scan[0][i] = key != CM_NONE && (i == 0 || (buf[i - 1] >> 32) != (key >> 32));
  }
  int cur = 0;
  for (int off = 1; off < ROWS_PER_BLOCK; off <<= 1) {                  // inclusive scan of the segment heads
    __syncthreads();
    for (int i = tid; i < ROWS_PER_BLOCK; i += 256) scan[cur ^ 1][i] = scan[cur][i] + (i >= off ? scan[cur][i - off] : 0);
    cur ^= 1;
  }
  __syncthreads();
  if (tid == 0 && buf[0] == CM_NONE) { nseg[b] = 0; nvalid[b] = 0; }
  for (int i = tid; i < ROWS_PER_BLOCK; i += 256) {
    const unsigned long long key = buf[i];
    if (key == CM_NONE) continue;
    const int s = scan[cur][i] - 1;
    order[r0 + i] = (int)(r0 + (long)(key & 0xFFFFFFFFull));
    if (i == 0 || (buf[i - 1] >> 32) != (key >> 32)) { seg_label[(long)b * segs + s] = (int)(key >> 32); seg_start[(long)b * segs + s] = i; }
    if (i == ROWS_PER_BLOCK - 1 || buf[i + 1] == CM_NONE) { nseg[b] = s + 1; nvalid[b] = i + 1; }
  }
}

__global__ __launch_bounds__(256) void wide_segment_sum_kernel(const float* __restrict__ x, int d, int segs, const int* __restrict__ order,
                                                                const int* __restrict__ seg_start, const int* __restrict__ nseg, const int* __restrict__ nvalid,
                                                                double* __restrict__ part /*[block][segs][d]*/) {
  const int b = blockIdx.x, ns = nseg[b], nv = nvalid[b];
  const long r0 = (long)b * ROWS_PER_BLOCK;
  for (int e = threadIdx.x; e < ns * d; e += 256) {
    const int sg = e / d, t = e - sg * d;
    const int st = seg_start[(long)b * segs + sg], en = sg + 1 < ns ? seg_start[(long)b * segs + sg + 1] : nv;
    double p = 0.0;
    for (int i = st; i < en; ++i) p += (double)x[(long)order[r0 + i] * d + t];      // the segment's rows in row order
    part[((long)b * segs + sg) * d + t] = p;
  }
}

// cluster j's segment in each of the blocks b0 + tid: the hits in block order -> l_seg (block * segs + slot), l_pos (first entry in `order`),
// l_len; returns their number to every thread.  Starts with a barrier, so the lists of the call before may be read up to it.
__device__ __noinline__ int wide_find_segments(int j, long b0, long nblk, int segs, const int* __restrict__ seg_label, const int* __restrict__ seg_start,
                                               const int* __restrict__ nseg, const int* __restrict__ nvalid, long* l_seg, int* l_pos, int* l_len, int* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long b = b0 + tid;
  int slot = -1, len = 0, start = 0;
  if (b < nblk) {
    const int ns = nseg[b];
    const int* sl = seg_label + b * segs;
    int lo = 0, hi = ns;                                                // first entry >= j
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (sl[mid] < j) lo = mid + 1; else hi = mid; }
    if (lo < ns && sl[lo] == j) {
      slot = lo;
      start = seg_start[b * segs + lo];
      len = (lo + 1 < ns ? seg_start[b * segs + lo + 1] : nvalid[b]) - start;
    }
  }
  const unsigned long long bal = __ballot(slot >= 0);
  __syncthreads();
  if (lane == 0) wsum[w] = __popcll(bal);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { const int v = wsum[q]; if (q < w) off += v; tot += v; }
  if (slot >= 0) {
    const int p = off + __popcll(bal & ((1ull << lane) - 1ull));
    l_seg[p] = b * segs + slot; l_pos[p] = (int)(b * ROWS_PER_BLOCK) + start; l_len[p] = len;
  }
  __syncthreads();
  return tot;
}

__global__ __launch_bounds__(256) void kmeans_update_wide_kernel(const double* __restrict__ part, int segs, const int* __restrict__ seg_label,
                                                                  const int* __restrict__ seg_start, const int* __restrict__ nseg, const int* __restrict__ nvalid,
                                                                  long nblk, int k, int d, float* __restrict__ cent, float* __restrict__ c2,
                                                                  float* __restrict__ counts, float* __restrict__ totalcounts) {
  __shared__ double red[256];
  __shared__ long l_seg[256];
  __shared__ int l_pos[256], l_len[256], wsum[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  int cnt = 0;
  double sm = 0.0;                                                      // column tid (d <= 256): the partials in block order
  for (long b0 = 0; b0 < nblk; b0 += 256) {
    const int nl = wide_find_segments(j, b0, nblk, segs, seg_label, seg_start, nseg, nvalid, l_seg, l_pos, l_len, wsum);
    for (int q0 = 0; q0 < nl; q0 += 8) {                                // eight loads in flight, then the adds in block order
      double p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = (q0 + u < nl && tid < d) ? part[l_seg[q0 + u] * d + tid] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (q0 + u < nl) { cnt += l_len[q0 + u]; if (tid < d) sm += p[u]; }
    }
  }
  double sq = 0.0;
  if (tid < d) {
    float v = cent[(long)j * d + tid];
    if (cnt != 0) {
      v = (float)sm / (float)cnt;                                       // kmeans_update_kernel's rounding
      cent[(long)j * d + tid] = v;
    }
    const float p = v * v;
    sq += (double)p;
  }
  red[tid] = sq;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;                                                   // thread order is column order (d <= 256), as in kmeans_update_kernel
    for (int t = 0; t < 256; ++t) tot += red[t];
    c2[j] = (float)tot * 0.5f;
    counts[j] = (float)cnt;
    totalcounts[j] += (float)cnt;
  }
}

__global__ __launch_bounds__(256) void cluster_members_wide_kernel(const int* __restrict__ order, int segs, const int* __restrict__ seg_label,
                                                                    const int* __restrict__ seg_start, const int* __restrict__ nseg, const int* __restrict__ nvalid,
                                                                    long nblk, const float* __restrict__ sims, int m, long* __restrict__ rows_out,
                                                                    float* __restrict__ sims_out, int* __restrict__ kept_out, int* __restrict__ sizes_out) {
  __shared__ unsigned long long buf[CM_BUF];
  __shared__ long l_seg[256];
  __shared__ int l_pos[256], l_len[256], wsum[4];
  __shared__ int s_count;
  const int j = blockIdx.x, tid = threadIdx.x;
  buf[tid] = CM_NONE; buf[tid + 256] = CM_NONE;
  if (tid == 0) s_count = 0;
  int count = 0, size = 0;                                              // count: keys in buf (the same number in every thread)
  unsigned long long thr = CM_NONE;                                     // the m-th smallest key so far, once m are known
  for (long b0 = 0; b0 < nblk; b0 += 256) {
    const int nl = wide_find_segments(j, b0, nblk, segs, seg_label, seg_start, nseg, nvalid, l_seg, l_pos, l_len, wsum);
    for (int q = 0; q < nl; ++q) size += l_len[q];
    const int pos = tid < nl ? l_pos[tid] : 0, len = tid < nl ? l_len[tid] : 0;
    for (int r = 0; __syncthreads_or(r < len); ++r) {                   // thread = segment; at most 256 keys join per round
      if (r < len) {
        const int row = order[pos + r];
        const unsigned long long kk = cm_key(sims[row], row);
        if (kk < thr) buf[atomicAdd(&s_count, 1)] = kk;                 // an integer counter: the set in buf does not depend on the order
      }
      __syncthreads();
      count = s_count;
      if (count > CM_BUF - 256) {                                       // the next round might not fit: sort, keep the m smallest
        cm_sort<CM_BUF>(buf, tid);
        count = min(count, m);
        if (tid >= count) buf[tid] = CM_NONE;
        buf[tid + 256] = CM_NONE;
        if (tid == 0) s_count = count;
        __syncthreads();
        if (count == m) thr = buf[m - 1];
      }
    }
  }
  cm_sort<CM_BUF>(buf, tid);
  const int kept = min(size, m);
  for (int e = tid; e < m; e += 256) {
    const long row = e < kept ? (long)(buf[e] & 0xFFFFFFFFull) : -1;
    rows_out[(long)j * m + e] = row;
    sims_out[(long)j * m + e] = e < kept ? sims[row] : 0.f;
  }
  if (tid == 0) { kept_out[j] = kept; sizes_out[j] = size; }
}

static int wide_segs(int k) { return min(k, KW_SEGMAX); }
bool cluster_takes_wide_route(int d, int k) { return k >= g_cluster_wide_min_k || k > KM_KMAX || (size_t)k * d * sizeof(double) > 60 * 1024; }
// narrow: the three launch_* workspaces one after the other; wide: k-means labels [n], order [blocks * 512], three ints per segment slot, two per
// block, one fp64 partial per (segment slot, column) - segment slots = blocks * min(k, 512), blocks = ceil(n / 512)
size_t cluster_workspace_bytes(long n, int d, int k) {
  const size_t a = 256;
  if (!cluster_takes_wide_route(d, k))
    return ((kmeans_workspace_bytes(n, d, k) + a - 1) / a + (cluster_members_workspace_bytes(n, k) + a - 1) / a) * a;
  const size_t nblk = (size_t)row_blocks(n), slots = nblk * wide_segs(k);
  return sizeof(double) * slots * d + sizeof(int) * (2 * slots + 2 * nblk + nblk * ROWS_PER_BLOCK + (size_t)n) + 8 * a;
}
// The wide route's member lists, shared by launch_cluster and gr_cluster_members_wide_dev (a mixture's labels and posteriors): the labels are grouped
// block by block (wide_group_kernel), then every cluster walks its segments (cluster_members_wide_kernel).  The index: three ints per segment slot,
// two per block, one per row of the padded table.
static size_t wide_align(size_t bytes) { return (bytes + 255) / 256 * 256; }
int wide_index_segs(int k) { return wide_segs(k); }
WideIndex wide_index_carve(char*& ws, long n, int k) {
  const size_t nblk = (size_t)row_blocks(n), slots = nblk * wide_segs(k);
  auto take = [&](size_t bytes) { char* p = ws; ws += wide_align(bytes); return reinterpret_cast<int*>(p); };
  WideIndex ix;
  ix.seg_label = take(sizeof(int) * slots);
  ix.seg_start = take(sizeof(int) * slots);
  ix.nseg = take(sizeof(int) * nblk);
  ix.nvalid = take(sizeof(int) * nblk);
  ix.order = take(sizeof(int) * nblk * ROWS_PER_BLOCK);
  return ix;
}
int wide_group(const int* labels, long n, int k, const WideIndex& ix, hipStream_t s) {
  KtScope kt("wide_group_kernel", 0.0, 8.0 * n, s);
  hipLaunchKernelGGL(wide_group_kernel, dim3((unsigned)row_blocks(n)), dim3(256), 0, s, labels, n, k, wide_segs(k), ix.order, ix.seg_label, ix.seg_start, ix.nseg, ix.nvalid);
  return 0;
}
static void wide_members(const int* labels, const float* sims, long n, int k, int m, long* rows_out, float* sims_out, int* kept_out, int* sizes_out,
                         const WideIndex& ix, hipStream_t s) {
  wide_group(labels, n, k, ix, s);
  KtScope kt("cluster_members_wide_kernel", 0.0, 12.0 * n, s);
  hipLaunchKernelGGL(cluster_members_wide_kernel, dim3(k), dim3(256), 0, s, ix.order, wide_segs(k), ix.seg_label, ix.seg_start, ix.nseg, ix.nvalid,
                     row_blocks(n), sims, m, rows_out, sims_out, kept_out, sizes_out);
}
size_t wide_index_bytes(long n, int k) {
  const size_t nblk = (size_t)row_blocks(n), slots = nblk * wide_segs(k);
  return sizeof(int) * (2 * slots + 2 * nblk + nblk * ROWS_PER_BLOCK) + 8 * 256;
}
size_t cluster_members_wide_workspace_bytes(long n, int k) { return wide_index_bytes(n, k); }
// launch_cluster_members' lists for any k <= 4096 by the wide route's kernels.  Returns 1 outside 1 <= k <= 4096, 1 <= m <= 128, 1 <= n < 2^31.
int launch_cluster_members_wide(const int* labels, const float* sims, long n, int k, int m, long* rows_out, float* sims_out, int* kept_out, int* sizes_out,
                                void* workspace, hipStream_t s) {
  if (k < 1 || k > KW_KMAX || m < 1 || m > CM_MMAX || n < 1 || n > 0x7FFFFFFFL) return 1;
  char* ws = static_cast<char*>(workspace);
  const WideIndex ix = wide_index_carve(ws, n, k);
  wide_members(labels, sims, n, k, m, rows_out, sims_out, kept_out, sizes_out, ix, s);
  return 0;
}
// apply_r.lua:198-227 in one enqueue; c2 / counts / w32 [k] scratch, totalcounts [k]; workspace from cluster_workspace_bytes.  Returns 1 outside
// 1 <= k <= 4096, d <= 256, 1 <= m <= 128, 1 <= n < 2^31, and 2 when the device refuses the assignment kernel's LDS.
int launch_cluster(const float* x, long n, int d, int k, int niter, float* cent, int take_min, int m, float* c2, float* counts, float* totalcounts,
                   float* w32, int* labels, float* sims, long* rows_out, float* sims_out, int* kept_out, int* sizes_out, void* workspace, hipStream_t s) {
  if (k < 1 || k > KW_KMAX || d < 1 || d > 256 || m < 1 || m > CM_MMAX || n < 1 || n > 0x7FFFFFFFL) return 1;
  const size_t a = 256;
  char* ws = static_cast<char*>(workspace);
  if (!cluster_takes_wide_route(d, k)) {
    void* ws_members = ws + (kmeans_workspace_bytes(n, d, k) + a - 1) / a * a;
    if (launch_kmeans(x, n, d, k, niter, cent, c2, counts, totalcounts, nullptr, ws, s)) return 1;
    if (launch_cosine_assign(x, n, d, cent, k, take_min, w32, labels, sims, s)) return 1;
    return launch_cluster_members(labels, sims, n, k, m, rows_out, sims_out, kept_out, sizes_out, ws_members, s);
  }
  const long nblk = row_blocks(n);
  const int segs = wide_segs(k);
  const size_t slots = (size_t)nblk * segs;
  auto take = [&](size_t bytes) { char* p = ws; ws += (bytes + a - 1) / a * a; return p; };
  double* part = reinterpret_cast<double*>(take(sizeof(double) * slots * d));
  const WideIndex ix = wide_index_carve(ws, n, k);
  int* klab = reinterpret_cast<int*>(take(sizeof(int) * (size_t)n));
  const size_t lds = sizeof(float) * KW_TR * (size_t)(d | 1);
  if (lds > 48 * 1024)                                                   // (per device; a host-side setting, cheap to repeat)
    for (const void* f : {reinterpret_cast<const void*>(kmeans_assign_wide_kernel), reinterpret_cast<const void*>(cosine_assign_wide_kernel)})
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * KW_TR * 257)) != hipSuccess) return 2;
  (void)hipMemsetAsync(totalcounts, 0, sizeof(float) * k, s);
  hipLaunchKernelGGL(kmeans_c2_kernel, dim3((k + 63) / 64), dim3(64), 0, s, cent, k, d, c2);
  for (int it = 0; it < niter; ++it) {
    { KtScope kt("kmeans_assign_wide_kernel", 2.0 * n * d * k, 4.0 * n * d, s);
      hipLaunchKernelGGL(kmeans_assign_wide_kernel, dim3((unsigned)((n + KW_TR - 1) / KW_TR)), dim3(256), lds, s, x, n, d, cent, c2, k, klab); }
    wide_group(klab, n, k, ix, s);
    { KtScope kt("wide_segment_sum_kernel", (double)n * d, 4.0 * n * d, s);
      hipLaunchKernelGGL(wide_segment_sum_kernel, dim3((unsigned)nblk), dim3(256), 0, s, x, d, segs, ix.order, ix.seg_start, ix.nseg, ix.nvalid, part); }
    KtScope kt("kmeans_update_wide_kernel", 0.0, 8.0 * n * d, s);
    hipLaunchKernelGGL(kmeans_update_wide_kernel, dim3(k), dim3(256), 0, s, part, segs, ix.seg_label, ix.seg_start, ix.nseg, ix.nvalid, nblk, k, d, cent, c2, counts, totalcounts);
  }
  hipLaunchKernelGGL(cosine_centroid_prep_kernel, dim3((k + 63) / 64), dim3(64), 0, s, cent, k, d, w32);
  { KtScope kt("cosine_assign_wide_kernel", 2.0 * n * d * k, 4.0 * n * d, s);
    hipLaunchKernelGGL(cosine_assign_wide_kernel, dim3((unsigned)((n + KW_TR - 1) / KW_TR)), dim3(256), lds, s, x, n, d, cent, w32, k, take_min, labels, sims); }
  wide_members(labels, sims, n, k, m, rows_out, sims_out, kept_out, sizes_out, ix, s);
  return 0;
}

}  // namespace gr
