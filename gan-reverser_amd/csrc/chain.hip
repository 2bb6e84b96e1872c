// chain.hip — the mean of n doubles in the library's fixed order (kernels.h, "the row-order chain"): what gr_vae_sample_dev's kl, gr_mixture_dev's
// loglik and gr_ssim_dev's mean are.  Compiled without FMA contraction like its callers (Makefile); there is no product here, only ordered adds.
//
// Kernels:
//   chain_mean_block_kernel  workgroup = block of ROWS_PER_BLOCK rows: the rows go to LDS, thread 0 adds them in row order from +0.0 -> one partial
//   chain_mean_join_kernel   ONE thread: the partials in block order from +0.0 (ordered_sum8), one division by n
// With one block the block kernel writes the mean itself and the join is not launched.  The bits are the join's: a block's sum starts from +0.0 and
// so is never -0.0, hence 0.0 + part[0] is part[0].
#include "kernels.h"

namespace gr {

__global__ __launch_bounds__(64) void chain_mean_block_kernel(const double* __restrict__ rows, long n, double* __restrict__ part, double* __restrict__ mean) {
  __shared__ double v[ROWS_PER_BLOCK];
  const long r0 = (long)blockIdx.x * ROWS_PER_BLOCK;
  const int nr = (int)min((long)ROWS_PER_BLOCK, n - r0);
  for (int e = threadIdx.x; e < nr; e += 64) v[e] = rows[r0 + e];
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int e = 0; e < nr; ++e) s = s + v[e];
    if (mean) *mean = s / (double)n;
    else part[blockIdx.x] = s;
  }
}

__global__ void chain_mean_join_kernel(const double* __restrict__ part, long nblk, long n, double* __restrict__ mean) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  *mean = ordered_sum8(part, nblk, 1) / (double)n;
}

void launch_chain_mean(const double* rows, long n, double* part, double* out, const char* timer, hipStream_t s) {
  const long nblk = row_blocks(n);
  KtScope kt(timer, (double)n, 8.0 * n, s);
  hipLaunchKernelGGL(chain_mean_block_kernel, dim3((unsigned)nblk), dim3(64), 0, s, rows, n, part, nblk == 1 ? out : nullptr);
  if (nblk > 1) hipLaunchKernelGGL(chain_mean_join_kernel, dim3(1), dim3(64), 0, s, part, nblk, n, out);
}

}  // namespace gr
