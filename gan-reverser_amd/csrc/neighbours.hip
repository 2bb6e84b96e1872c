// neighbours.hip — exact L2 nearest-neighbour search (reference sample.lua:130-148 findClosestNeighboursOf: torch.dist of every training
// image against each query, first minimum kept).  Contract (include/ganrev.h gr_l2_nearest_*): S(q, j) = sum over i, left to right in
// fp64, of (double)(t * t) with t = |x_ji - q_i| and t * t rounded to fp32; dist = sqrt(S) in fp64; the k smallest by (dist, row index).
// Compiled with -ffp-contract=off: t * t must stay a rounded fp32 product in every kernel here.
//   1. l2_approx_kernel:       ONE streaming pass over the table [n][d].  A wave takes ROWS rows at a time, lane l the columns
//                              l, l + 64, ... (16-byte loads); per (row, query) the lane sums the reference's own terms t * t in fp32,
//                              the 64 lane sums are combined in fp64 (a reduce-scatter over the lanes: one finished sum per lane) and
//                              S~ is written out (8 bytes per row and query: 0.2 % of the table's bytes at d = 1024).  Queries come
//                              through L2 in groups of at most 16, one pass over the table per group.
//   2. l2_select_kernel:       one workgroup per query, reads only S~: every thread's minimum over its rows, the k-th smallest of those
//                              1024 minima is tau0 (k distinct rows have S~ <= tau0); the rows with S~ <= tau0 (1 + 4 eps) are the
//                              candidates (at most CAND_MAX), re-scored exactly in the reference's order (one thread per candidate) and
//                              ranked by (dist, row).
//   3. l2_exact_kernel +       the exact path: every (row, query) scored in the reference's order, then a radix select of the k-th
//      l2_exact_select_kernel  smallest dist and the rows before it in (dist, row) order.  Taken outright for n <= DIRECT_ROWS, and when a
//                              candidate list overflowed (hundreds of exact copies of the nearest row, a constant table) or the sums
//                              approach the fp32 range (see below).
//
// Bound of the filter.  The terms t * t are exactly the reference's; only the summation differs.  All terms are >= 0, so every
// addition rounds with relative error <= u = 2^-24 (fp32: an addition whose result is subnormal is exact) resp. 2^-53 (fp64): a lane
// summing T terms is within gamma_T = T u / (1 - T u) of its exact sum, the fp64 combine adds 6 roundings, the reference's own
// sequential fp64 sum d of them.  With T <= 4 ceil(d / 256) + 4 <= 1028 (d <= 65536):
//     |S~ - S| <= eps S,   eps = (T + 2) * 2^-24 + (d + 64) * 2^-51          (l2_filter_eps, L2_TERM_ERR below)
// Any row of the exact k nearest has S <= S_(k) <= tau0 (1 + 2 eps), hence S~ <= tau0 (1 + 4 eps): it is a candidate.  A row that is
// not has S >= S~ / (1 + eps) > tau0 (1 + 2.9 eps) > S_(k) (1 + 2^-50): its dist is larger than the k-th's even after the rounding of
// sqrt, so it cannot tie in.  tau0 = 0 keeps exactly the rows with S = 0.
// Range.  A lane sum that overflows fp32 makes S~ = inf although S may be finite (S > 2^127 then); tau0 >= 2^126 (or NaN: fewer than k
// rows with a number) therefore keeps EVERY row, which overflows the list for any n > CAND_MAX and sends the call down the exact path.
// A NaN term makes S~ and S NaN alike; NaN orders after +inf (key 0x7FF8...).
#include "kernels.h"

namespace gr {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int L2_ROWS = 4;                 // rows per wave and round of l2_approx_kernel (their query values are loaded once)
constexpr int L2_QG = 16;                  // queries per pass over the table
constexpr int L2_CAND_MAX = 256;           // candidates a query may keep (expected ~k + k^2 / 2048 on random data); more: the exact path
constexpr long L2_DIRECT_ROWS = 4096;      // up to this many rows the exact path is taken outright
constexpr double L2_TERM_ERR = 5.9604644775390625e-08;     // 2^-24: relative rounding of one fp32 addition of non-negative terms
constexpr unsigned long long L2_KEY_NAN = 0x7FF8000000000000ull;
constexpr unsigned long long L2_KEY_HUGE = 0x47D0000000000000ull;   // 2^126 as a double's bits: tau0 at or above it keeps every row

static_assert(L2_CAND_MAX <= 1024, "one candidate per thread of l2_select_kernel");

double l2_filter_eps(int d, bool vec) {
  const long T = vec ? 4L * ((d / 4 + 63) / 64) : (long)((d + 63) / 64);
  return (double)(T + 2) * L2_TERM_ERR + (double)(d + 64) * 4.440892098500626e-16;
}

// an order-preserving key of a non-negative double or NaN (S and sqrt(S) are never negative; -0 does not occur: sums start at +0)
__device__ __forceinline__ unsigned long long l2_key(double v) {
  return v != v ? L2_KEY_NAN : (unsigned long long)__double_as_longlong(v);
}

// the reference's sum for one (row, query): left to right, fp32 terms, fp64 accumulator
__device__ __forceinline__ double l2_exact_sum(const float* __restrict__ xr, const float* __restrict__ qv, int d, bool vec) {
  double s = 0.0;
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(xr);
    const float4* q4 = reinterpret_cast<const float4*>(qv);
    const int d4 = d >> 2;
#pragma unroll 4
    for (int c = 0; c < d4; ++c) {
      const float4 a = x4[c], b = q4[c];
      float t;
      t = fabsf(a.x - b.x); s += (double)(t * t);
      t = fabsf(a.y - b.y); s += (double)(t * t);
      t = fabsf(a.z - b.z); s += (double)(t * t);
      t = fabsf(a.w - b.w); s += (double)(t * t);
    }
  } else {
    for (int i = 0; i < d; ++i) { const float t = fabsf(xr[i] - qv[i]); s += (double)(t * t); }
  }
  return s;
}

// V values per lane -> lane l holds the sum over all 64 lanes of value number (l >> (6 - log2 V)), in fp64.  Each level sends half of
// the values to the partner lane and keeps the other half: 2 V - 2 shuffles in all instead of 6 V for V separate trees.
template <int M, int V>
__device__ __forceinline__ void l2_rs_level(double (&v)[V], int lane) {      // one level: M values left, partner lane ^ (32 M / V)
  if constexpr (M > 1) {
    constexpr int off = 32 * M / V;
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < M / 2; ++i) {
      const double send = hi ? v[i] : v[i + M / 2];
      const double keep = hi ? v[i + M / 2] : v[i];
      v[i] = keep + __shfl_xor(send, off, 64);
    }
    l2_rs_level<M / 2, V>(v, lane);
  }
}
template <int V>
__device__ __forceinline__ double l2_reduce_scatter(double (&v)[V], int lane) {
  static_assert(V >= 1 && V <= 64 && (V & (V - 1)) == 0, "V: a power of two <= 64");
  l2_rs_level<V, V>(v, lane);
  double r = v[0];
#pragma unroll
  for (int off = 32 / V; off > 0; off >>= 1) r += __shfl_xor(r, off, 64);
  return r;
}

// S~ for queries q0 .. q0 + nq - 1 (nq <= NQ; the padding slots repeat query q0 and are not written) of every row: akeys[q][row].
// Persistent: gridDim.x is one resident round; wave w takes the row groups w, w + waves, ...  Two rows share a packed fp32 register
// pair, so the difference, the square and the sum run as v_pk_add_f32 / v_pk_mul_f32 (the terms are still rounded like the reference's).
template <int NQ, bool VEC>
__global__ __launch_bounds__(256) void l2_approx_kernel(const float* __restrict__ x, long n, int d, const float* __restrict__ qs, int q0, int nq,
                                                        double* __restrict__ akeys) {
  constexpr int R = L2_ROWS, V = R * NQ;
  static_assert(R % 2 == 0, "rows go in pairs");
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = (long)gridDim.x * (blockDim.x >> 6);
  const long ngroups = (n + R - 1) / R;
  const float* qp[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) qp[j] = qs + (long)(q0 + (j < nq ? j : 0)) * d;
  for (long g = wave; g < ngroups; g += nwaves) {
    const float* xp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { const long row = g * R + r; xp[r] = x + (row < n ? row : n - 1) * (long)d; }
    f32x2 acc[R / 2][NQ];
#pragma unroll
    for (int p = 0; p < R / 2; ++p)
#pragma unroll
      for (int j = 0; j < NQ; ++j) acc[p][j] = f32x2{0.f, 0.f};
    if (VEC) {
      const int d4 = d >> 2;
      for (int c = lane; c < d4; c += 64) {
        float4 xv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) xv[r] = reinterpret_cast<const float4*>(xp[r])[c];
        f32x2 xe[R / 2][4];                       // (row 2p, row 2p + 1) of each of the 4 columns
#pragma unroll
        for (int p = 0; p < R / 2; ++p) {
          xe[p][0] = f32x2{xv[2 * p].x, xv[2 * p + 1].x}; xe[p][1] = f32x2{xv[2 * p].y, xv[2 * p + 1].y};
          xe[p][2] = f32x2{xv[2 * p].z, xv[2 * p + 1].z}; xe[p][3] = f32x2{xv[2 * p].w, xv[2 * p + 1].w};
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const float4 qv = reinterpret_cast<const float4*>(qp[j])[c];
          const float qe[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int p = 0; p < R / 2; ++p) { const f32x2 t = xe[p][e] - f32x2{qe[e], qe[e]}; acc[p][j] += t * t; }
        }
      }
    } else {
      for (int c = lane; c < d; c += 64) {
        f32x2 xe[R / 2];
#pragma unroll
        for (int p = 0; p < R / 2; ++p) xe[p] = f32x2{xp[2 * p][c], xp[2 * p + 1][c]};
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const float qv = qp[j][c];
#pragma unroll
          for (int p = 0; p < R / 2; ++p) { const f32x2 t = xe[p] - f32x2{qv, qv}; acc[p][j] += t * t; }
        }
      }
    }
    double v[V];                                  // value r * NQ + j: row g R + r, query j
#pragma unroll
    for (int p = 0; p < R / 2; ++p)
#pragma unroll
      for (int j = 0; j < NQ; ++j) { v[(2 * p) * NQ + j] = (double)acc[p][j].x; v[(2 * p + 1) * NQ + j] = (double)acc[p][j].y; }
    const double s = l2_reduce_scatter<V>(v, lane);
    constexpr int SH = V == 64 ? 0 : (V == 32 ? 1 : (V == 16 ? 2 : (V == 8 ? 3 : (V == 4 ? 4 : (V == 2 ? 5 : 6)))));
    const int vi = lane >> SH, r = vi / NQ, j = vi - r * NQ;
    const long row = g * R + r;
    if ((lane & ((1 << SH) - 1)) == 0 && j < nq && row < n) akeys[(long)(q0 + j) * n + row] = s;
  }
}

// Fast path's selection: one workgroup (1024 threads) per query over its S~ row akeys[q][.]; see the file header.  status[q] = 1 when the
// list overflowed (the caller takes the exact path), else 0 and the k results.
__global__ __launch_bounds__(1024) void l2_select_kernel(const float* __restrict__ x, long n, int d, const float* __restrict__ qs,
                                                         const double* __restrict__ akeys, int k, double win, int vec,
                                                         long* __restrict__ idx_out, double* __restrict__ dist_out, unsigned* __restrict__ status) {
  __shared__ unsigned long long sk[1024];
  __shared__ unsigned cand[L2_CAND_MAX];
  __shared__ unsigned long long dk[L2_CAND_MAX];
  __shared__ unsigned cnt;
  const int q = blockIdx.x, tid = threadIdx.x;
  const double* a = akeys + (long)q * n;
  unsigned long long mn = ~0ull;                  // (a thread without rows: above every key)
  for (long i = tid; i < n; i += 1024) { const unsigned long long kk = l2_key(a[i]); mn = kk < mn ? kk : mn; }
  sk[tid] = mn;
  if (tid == 0) cnt = 0u;
  __syncthreads();
  for (int size = 2; size <= 1024; size <<= 1)   // bitonic sort of the 1024 minima, ascending
    for (int st = size >> 1; st > 0; st >>= 1) {
      const int p = tid ^ st;
      if (p > tid) {
        const unsigned long long u = sk[tid], w = sk[p];
        if ((u > w) == ((tid & size) == 0)) { sk[tid] = w; sk[p] = u; }
      }
      __syncthreads();
    }
  const unsigned long long t0 = sk[k - 1];
  const bool all = t0 >= L2_KEY_HUGE;
  const double tau = all ? INFINITY : __longlong_as_double((long long)t0) * win;
  for (long i = tid; i < n; i += 1024) {
    const double s = a[i];
    if (all || s <= tau) { const unsigned pos = atomicAdd(&cnt, 1u); if (pos < (unsigned)L2_CAND_MAX) cand[pos] = (unsigned)i; }
  }
  __syncthreads();
  const unsigned m = cnt;
  if (m > (unsigned)L2_CAND_MAX || m < (unsigned)k) { if (tid == 0) status[q] = 1u; return; }
  const float* qv = qs + (long)q * d;
  if ((unsigned)tid < m) dk[tid] = l2_key(sqrt(l2_exact_sum(x + (long)cand[tid] * d, qv, d, vec != 0)));
  __syncthreads();
  if ((unsigned)tid < m) {                        // rank by (dist, row): rows are distinct, so the ranks are
    const unsigned long long mk = dk[tid]; const unsigned mr = cand[tid];
    int rank = 0;
    for (unsigned j = 0; j < m; ++j) { const unsigned long long o = dk[j]; rank += (o < mk || (o == mk && cand[j] < mr)) ? 1 : 0; }
    if (rank < k) { idx_out[(long)q * k + rank] = (long)mr; dist_out[(long)q * k + rank] = __longlong_as_double((long long)mk); }
  }
  if (tid == 0) status[q] = 0u;
}

// Exact path, step 1: dist key of every (row, query) in the reference's order: ekeys[q][row]
__global__ __launch_bounds__(256) void l2_exact_kernel(const float* __restrict__ x, long n, int d, const float* __restrict__ qs, int vec,
                                                       unsigned long long* __restrict__ ekeys) {
  const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = blockIdx.y;
  if (row >= n) return;
  ekeys[(long)q * n + row] = l2_key(sqrt(l2_exact_sum(x + row * (long)d, qs + (long)q * d, d, vec != 0)));
}

// Exact path, step 2 (one workgroup of 1024 per query): radix select (8 bits per round) of the k-th smallest key v; the rows with
// key < v (fewer than k: gathered in any order) and the first rows with key == v in row order fill the k places; ranked by (dist, row).
__global__ __launch_bounds__(1024) void l2_exact_select_kernel(const unsigned long long* __restrict__ ekeys, long n, int k,
                                                               long* __restrict__ idx_out, double* __restrict__ dist_out) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long lk[128];
  __shared__ unsigned lr[128];
  __shared__ unsigned wsum[16];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_rank, s_n, s_need;
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long* e = ekeys + (long)q * n;
  unsigned long long prefix = 0ull, mask = 0ull;
  unsigned rank = (unsigned)k;                    // 1-based rank of the wanted key among the keys matching prefix
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += 1024) hist[i] = 0u;
    __syncthreads();
    for (long i = tid; i < n; i += 1024) { const unsigned long long kk = e[i]; if ((kk & mask) == prefix) atomicAdd(&hist[(unsigned)(kk >> shift) & 255u], 1u); }
    __syncthreads();
    if (tid == 0) {
      unsigned cum = 0u; int b = 0;
      for (; b < 255; ++b) { if (cum + hist[b] >= rank) break; cum += hist[b]; }
      s_prefix = prefix | ((unsigned long long)b << shift); s_rank = rank - cum;
    }
    __syncthreads();
    prefix = s_prefix; rank = s_rank; mask |= 0xFFull << shift;
    __syncthreads();
  }
  const unsigned long long v = prefix;            // the k-th smallest key; `rank` rows with key == v are wanted
  if (tid == 0) { s_n = 0u; s_need = rank; }
  __syncthreads();
  for (long i = tid; i < n; i += 1024) { const unsigned long long kk = e[i]; if (kk < v) { const unsigned p = atomicAdd(&s_n, 1u); lk[p] = kk; lr[p] = (unsigned)i; } }
  __syncthreads();
  for (long t0 = 0; t0 < n; t0 += 1024) {         // rows with key == v, in row order, until `rank` of them are in
    if (s_need == 0u) break;                      // (uniform: read after the barrier that ended the last round)
    const long i = t0 + tid;
    const bool hit = i < n && e[i] == v;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) wsum[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += wsum[w];
    const unsigned need = s_need, base = s_n;
    if (hit && before < need) { lk[base + before] = v; lr[base + before] = (unsigned)i; }
    __syncthreads();
    if (tid == 0) { unsigned tot = 0u; for (int w = 0; w < 16; ++w) tot += wsum[w]; const unsigned take = tot < need ? tot : need; s_n = base + take; s_need = need - take; }
    __syncthreads();
  }
  if (tid < k) {
    const unsigned long long mk = lk[tid]; const unsigned mr = lr[tid];
    int r = 0;
    for (int j = 0; j < k; ++j) { const unsigned long long o = lk[j]; r += (o < mk || (o == mk && lr[j] < mr)) ? 1 : 0; }
    idx_out[(long)q * k + r] = (long)mr; dist_out[(long)q * k + r] = __longlong_as_double((long long)mk);
  }
}

size_t l2_nearest_workspace_bytes(long n, int Q) { return sizeof(double) * (size_t)n * Q; }

template <int NQ, bool VEC>
static void launch_approx(const float* x, long n, int d, const float* qs, int q0, int nq, double* akeys, int num_cus, hipStream_t s) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&l2_approx_kernel<NQ, VEC>), 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  long grid = (long)num_cus * per_cu;                           // one resident round
  const long need = ((n + L2_ROWS - 1) / L2_ROWS + 3) / 4;       // (a workgroup per 4 row groups at most)
  if (grid > need) grid = need;
  hipLaunchKernelGGL((l2_approx_kernel<NQ, VEC>), dim3((unsigned)grid), dim3(256), 0, s, x, n, d, qs, q0, nq, akeys);
}
template <bool VEC>
static void launch_approx_nq(int nq, const float* x, long n, int d, const float* qs, int q0, double* akeys, int num_cus, hipStream_t s) {
  if (nq <= 1) launch_approx<1, VEC>(x, n, d, qs, q0, nq, akeys, num_cus, s);
  else if (nq <= 2) launch_approx<2, VEC>(x, n, d, qs, q0, nq, akeys, num_cus, s);
  else if (nq <= 4) launch_approx<4, VEC>(x, n, d, qs, q0, nq, akeys, num_cus, s);
  else if (nq <= 8) launch_approx<8, VEC>(x, n, d, qs, q0, nq, akeys, num_cus, s);
  else launch_approx<16, VEC>(x, n, d, qs, q0, nq, akeys, num_cus, s);
}

bool l2_nearest_direct(long n) { return n <= L2_DIRECT_ROWS; }

int launch_l2_nearest(const float* x, long n, int d, const float* qs, int Q, int k, long* idx_out, double* dist_out, unsigned* status,
                      void* workspace, int exact, int num_cus, hipStream_t s) {
  if (n < 1 || n >= 0xFFFFFFFFl || d < 1 || d > 65536 || Q < 1 || k < 1 || k > 128 || k > n) return -1;
  const bool vec = (d & 3) == 0 && aligned16(x) && aligned16(qs);
  if (exact) {
    unsigned long long* ekeys = reinterpret_cast<unsigned long long*>(workspace);
    {
      KtScope kt("l2_exact_kernel", 3.0 * n * d * Q, 4.0 * n * d * Q, s);
      hipLaunchKernelGGL(l2_exact_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)Q), dim3(256), 0, s, x, n, d, qs, (int)vec, ekeys);
    }
    KtScope kt("l2_exact_select_kernel", 0.0, 8.0 * 9 * n * Q, s);
    hipLaunchKernelGGL(l2_exact_select_kernel, dim3((unsigned)Q), dim3(1024), 0, s, ekeys, n, k, idx_out, dist_out);
    return 0;
  }
  double* akeys = reinterpret_cast<double*>(workspace);
  for (int q0 = 0; q0 < Q; q0 += L2_QG) {
    const int nq = Q - q0 < L2_QG ? Q - q0 : L2_QG;
    KtScope kt("l2_approx_kernel", 3.0 * n * d * nq, 4.0 * n * d + 8.0 * n * nq, s);
    if (vec) launch_approx_nq<true>(nq, x, n, d, qs, q0, akeys, num_cus, s);
    else launch_approx_nq<false>(nq, x, n, d, qs, q0, akeys, num_cus, s);
  }
  const double win = 1.0 + 4.0 * l2_filter_eps(d, vec);
  KtScope kt("l2_select_kernel", 0.0, 16.0 * n * Q, s);
  hipLaunchKernelGGL(l2_select_kernel, dim3((unsigned)Q), dim3(1024), 0, s, x, n, d, qs, akeys, k, win, (int)vec, idx_out, dist_out, status);
  return 0;
}

}  // namespace gr
