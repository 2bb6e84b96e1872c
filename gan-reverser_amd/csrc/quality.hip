// quality.hip — image-to-image scores on device tensors (gr_ssim_dev: the structural similarity index of Wang et al. 2004 and the mean squared error
// of the same pass; new: no counterpart in the reference, whose README names regression to the mean, which L2 rewards, as the fix-faces loop's artefact).
// a, b [n x C x h x w] floats.
//
// The arithmetic is stated in include/ganrev.h and restated in numpy in ganrev/quality.py; this file is compiled without FMA contraction (Makefile), so
// every multiply and add below rounds on its own.  Everything past the loads is fp64: the floats enter by an exact conversion, and a product of two
// of them is exact.  No floating-point atomics, no grid barrier, nothing sized by the CU count: every result is a function of the inputs alone.
//
// Operation by operation (all fp64; g[0 .. win) the 1-D window, formed on the host):
//   horizontal  per input row i and valid column c, five chains over t = 0 .. win - 1 from +0.0:  H = H + g[t] q[i][c + t],
//               q = x, y, x x, y y, x y  (x = a, y = b)
//   vertical    per valid position (r, c), five chains over t from +0.0:  V = V + g[t] H[r + t][c]  ->  mx, my, sxx, syy, sxy
//   position    mxx = mx mx, myy = my my, mxy = mx my;  vx = sxx - mxx, vy = syy - myy, cxy = sxy - mxy
//               n1 = 2 mxy + C1, n2 = 2 cxy + C2, d1 = (mxx + myy) + C1, d2 = (vx + vy) + C2;  S = (n1 n2) / (d1 d2)
//   image       R_r = the S of row r in column order from +0.0; P_ch = the R_r in row order from +0.0; Q = the P_ch in channel order from +0.0;
//               q = Q / (C oh ow); ssim_rows = (float)q.  mse_rows the same way over every pixel with e = d d, d = x - y, divided by C h w
//   mean        per block of 512 consecutive images the q in image order from +0.0, the block partials in block order from +0.0, one division by n
// x and y go through the same instructions, and every operation that mixes them is commutative: swapping a and b gives the same bits, and a == b
// gives n1 == d1, n2 == d2 bit for bit (2 m = m + m exactly), so S == 1.
//
// Kernels:
//   ssim_image_kernel<WIN>   workgroup = one image (grid-stride over images), the channels and, inside a channel, strips of rows looped.  A strip's rows
//                            of both planes go to LDS as floats (16-byte loads when `vec`, the same bits), odd pitch; the horizontal pass writes five
//                            fp64 planes to LDS, the vertical pass reads them (thread = one position, neighbours = neighbouring columns: no bank is
//                            shared) and leaves S in LDS at an odd pitch, where thread = row adds its row.  A strip holds as many rows as the LDS
//                            budget admits (ssim_plan); strips overlap by win - 1 rows, whose horizontal pass is repeated.  The sums R_r wait in LDS
//                            until the channel is done, so no result depends on the strip height.
//   (chain.hip, launch_chain_mean)   mean[0] from the q
// Roughly 4 win (h ow + oh ow) 5 fp64 operations per channel against 8 h w bytes read: compute- and LDS-bound, not bandwidth-bound.
#include "kernels.h"

namespace gr {

constexpr int SQ_MAX_HW = 128;                // h and w at most
constexpr int SQ_MAX_WIN = 11;
constexpr size_t SQ_LDS_SMALL = 64 * 1024, SQ_LDS_LARGE = 144 * 1024;      // the budget of a strip: the larger one only where the smaller gives short strips

struct SsimWindow { double g[SQ_MAX_WIN]; };

// The LDS image of a strip of `rows` input rows (floats fa, fb at pitch fp; doubles H[5] at pitch ow, S at pitch sp, the row sums R [oh] and E [h])
struct SsimPlan { int rows, fp, sp; size_t bytes; };

static size_t ssim_row_bytes(int ow, int fp, int sp) { return 2 * sizeof(float) * (size_t)fp + sizeof(double) * (5 * (size_t)ow + (size_t)sp); }
static size_t ssim_fixed_bytes(int h, int oh) { return sizeof(double) * (size_t)(h + oh) + 16; }

static SsimPlan ssim_plan(int h, int w, int win) {
  const int ow = w - win + 1, oh = h - win + 1;
  SsimPlan p;
  p.fp = w | 1; p.sp = ow | 1;
  const size_t rb = ssim_row_bytes(ow, p.fp, p.sp), fixed = ssim_fixed_bytes(h, oh);
  const int want = h < 2 * win ? h : 2 * win;
  int rows = (int)((SQ_LDS_SMALL - fixed) / rb);
  if (rows < want) rows = (int)((SQ_LDS_LARGE - fixed) / rb);       // >= 20 at the cap (h = w = 128, win = 3: 7080 bytes a row)
  p.rows = rows < h ? rows : h;
  p.bytes = fixed + rb * (size_t)p.rows;
  return p;
}

template <int WIN>
__global__ __launch_bounds__(256) void ssim_image_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, int C, int h, int w, int strip, int fp,
                                                          int sp, int vec, SsimWindow win, double c1, double c2, float* __restrict__ ssim_rows,
                                                          float* __restrict__ mse_rows, double* __restrict__ rowq) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int ow = w - WIN + 1, oh = h - WIN + 1;
  // carve: doubles first (8-byte aligned throughout), the floats last
  double* H = reinterpret_cast<double*>(smem);                         // [5][strip][ow]
  double* S = H + 5 * (size_t)strip * ow;                              // [strip][sp] (strip - WIN + 1 rows used)
  double* R = S + (size_t)strip * sp;                                  // [oh]
  double* E = R + oh;                                                  // [h]
  float* fa = reinterpret_cast<float*>(E + h);                         // [strip][fp]
  float* fb = fa + (size_t)strip * fp;
  const long hplane = (long)strip * ow;
  const int step = strip - WIN + 1;                                    // output rows per strip (>= 1: strip >= WIN)

  for (long img = blockIdx.x; img < n; img += gridDim.x) {
    double qs = 0.0, qe = 0.0;                                         // Q of the SSIM (thread 0) and of the squared error (thread 64)
    for (int ch = 0; ch < C; ++ch) {
      const float* pa = a + (img * C + ch) * (long)h * w;
      const float* pb = b + (img * C + ch) * (long)h * w;
      int seen = 0;                                                    // input rows whose squared error is summed already
      for (int o0 = 0; o0 < oh; o0 += step) {
        const int no = min(step, oh - o0);                             // output rows of this strip
        const int nr = no + WIN - 1;                                   // input rows o0 .. o0 + nr - 1 (<= h - 1)
        // 1. the strip's rows of both planes
        if (vec) {
          const int nq = w >> 2;
          for (int e = tid; e < nr * nq; e += 256) {
            const int i = e / nq, c = (e - i * nq) * 4;
            const float4 va = *reinterpret_cast<const float4*>(pa + (long)(o0 + i) * w + c);
            const float4 vb = *reinterpret_cast<const float4*>(pb + (long)(o0 + i) * w + c);
            float* da = fa + i * fp + c; float* db = fb + i * fp + c;
            da[0] = va.x; da[1] = va.y; da[2] = va.z; da[3] = va.w;
            db[0] = vb.x; db[1] = vb.y; db[2] = vb.z; db[3] = vb.w;
          }
        } else {
          for (int e = tid; e < nr * w; e += 256) {
            const int i = e / w, c = e - i * w;
            fa[i * fp + c] = pa[(long)(o0 + i) * w + c];
            fb[i * fp + c] = pb[(long)(o0 + i) * w + c];
          }
        }
        __syncthreads();
        // 2. horizontal pass: thread = (row, valid column)
        for (int e = tid; e < nr * ow; e += 256) {
          const int i = e / ow, c = e - i * ow;
          const float* ra = fa + i * fp + c; const float* rb = fb + i * fp + c;
          double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
          for (int t = 0; t < WIN; ++t) {
            const double x = (double)ra[t], y = (double)rb[t], g = win.g[t];
            hx = hx + g * x;
            hy = hy + g * y;
            hxx = hxx + g * (x * x);
            hyy = hyy + g * (y * y);
            hxy = hxy + g * (x * y);
          }
          double* d = H + (long)i * ow + c;
          d[0] = hx; d[hplane] = hy; d[2 * hplane] = hxx; d[3 * hplane] = hyy; d[4 * hplane] = hxy;
        }
        //    and the squared error of the rows no earlier strip held: thread = row, in column order
        if (mse_rows && tid >= 128 && tid - 128 < nr && o0 + (tid - 128) >= seen) {
          const int i = tid - 128;
          double s = 0.0;
          for (int c = 0; c < w; ++c) {
            const double d = (double)fa[i * fp + c] - (double)fb[i * fp + c];
            s = s + d * d;
          }
          E[o0 + i] = s;
        }
        seen = o0 + nr;
        __syncthreads();
        // 3. vertical pass and the index of each valid position
        for (int e = tid; e < no * ow; e += 256) {
          const int r = e / ow, c = e - r * ow;
          const double* s = H + (long)r * ow + c;
          double mx = 0.0, my = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
          for (int t = 0; t < WIN; ++t) {
            const double g = win.g[t];
            const double* q = s + (long)t * ow;
            mx = mx + g * q[0];
            my = my + g * q[hplane];
            sxx = sxx + g * q[2 * hplane];
            syy = syy + g * q[3 * hplane];
            sxy = sxy + g * q[4 * hplane];
          }
          const double mxx = mx * mx, myy = my * my, mxy = mx * my;
          const double vx = sxx - mxx, vy = syy - myy, cxy = sxy - mxy;
          const double n1 = 2.0 * mxy + c1;
          const double n2 = 2.0 * cxy + c2;
          const double d1 = (mxx + myy) + c1;
          const double d2 = (vx + vy) + c2;
          S[r * sp + c] = (n1 * n2) / (d1 * d2);
        }
        __syncthreads();
        // 4. thread = output row adds its row in column order
        if (tid < no) {
          double s = 0.0;
          for (int c = 0; c < ow; ++c) s = s + S[tid * sp + c];
          R[o0 + tid] = s;
        }
        __syncthreads();
      }
      // the channel: rows in order, then onto the channels before it (two threads of different waves, side by side)
      if (tid == 0) {
        double p = 0.0;
        for (int r = 0; r < oh; ++r) p = p + R[r];
        qs = qs + p;
      }
      if (tid == 64 && mse_rows) {
        double p = 0.0;
        for (int r = 0; r < h; ++r) p = p + E[r];
        qe = qe + p;
      }
      // (the next channel's R and E are written behind barriers that these two threads reach only after their sums)
    }
    if (tid == 0) {
      const double q = qs / (double)((long)C * oh * ow);
      ssim_rows[img] = (float)q;
      if (rowq) rowq[img] = q;
    }
    if (tid == 64 && mse_rows) mse_rows[img] = (float)(qe / (double)((long)C * h * w));
  }
}

// ------------------------------------------------------------------ launchers
bool ssim_args_ok(long n, int channels, int h, int w, int win) {
  return n >= 1 && n <= 0x7FFFFFFFL && channels >= 1 && win >= 3 && win <= SQ_MAX_WIN && (win & 1) && h >= win && w >= win &&
         h <= SQ_MAX_HW && w <= SQ_MAX_HW;
}

template <int WIN>
static int ssim_launch_image(const float* a, const float* b, long n, int C, int h, int w, const SsimPlan& p, int vec, const SsimWindow& g, double c1, double c2,
                             float* ssim_rows, float* mse_rows, double* rowq, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ssim_image_kernel<WIN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SQ_LDS_LARGE) != hipSuccess) return 2;
    attr = true;
  }
  const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
  const double ow = w - WIN + 1, oh = h - WIN + 1;
  KtScope kt("ssim_image_kernel", (double)n * C * (20.0 * WIN * (h * ow + oh * ow) + 3.0 * h * w), 8.0 * n * C * h * w, s);
  hipLaunchKernelGGL(ssim_image_kernel<WIN>, dim3(grid), dim3(256), p.bytes, s, a, b, n, C, h, w, p.rows, p.fp, p.sp, vec, g, c1, c2, ssim_rows, mse_rows, rowq);
  return 0;
}

// 1: outside the limits; 2: the device refuses the kernel's LDS.  sigma <= 0: the uniform window
int launch_ssim(const float* a, const float* b, long n, int channels, int h, int w, int win, double sigma, double data_range, float* ssim_rows, float* mse_rows,
                double* mean, void* workspace, hipStream_t s) {
  if (!ssim_args_ok(n, channels, h, w, win) || !(data_range > 0)) return 1;
  SsimWindow g;
  if (sigma > 0) {
    const double mid = (double)(win - 1) / 2.0, den = 2.0 * (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < win; ++i) { const double d = (double)i - mid; g.g[i] = std::exp(-(d * d) / den); sum = sum + g.g[i]; }
    for (int i = 0; i < win; ++i) g.g[i] = g.g[i] / sum;
  } else {
    for (int i = 0; i < win; ++i) g.g[i] = 1.0 / (double)win;
  }
  for (int i = win; i < SQ_MAX_WIN; ++i) g.g[i] = 0.0;
  const double k1 = 0.01 * data_range, k2 = 0.03 * data_range;
  const double c1 = k1 * k1, c2 = k2 * k2;
  const SsimPlan p = ssim_plan(h, w, win);
  if (p.rows < win || p.bytes > SQ_LDS_LARGE) return 1;
  const int vec = w % 4 == 0 && aligned16(a) && aligned16(b);
  double* rowq = mean ? reinterpret_cast<double*>(workspace) : nullptr;
  int r;
  switch (win) {
    case 3: r = ssim_launch_image<3>(a, b, n, channels, h, w, p, vec, g, c1, c2, ssim_rows, mse_rows, rowq, s); break;
    case 5: r = ssim_launch_image<5>(a, b, n, channels, h, w, p, vec, g, c1, c2, ssim_rows, mse_rows, rowq, s); break;
    case 7: r = ssim_launch_image<7>(a, b, n, channels, h, w, p, vec, g, c1, c2, ssim_rows, mse_rows, rowq, s); break;
    case 9: r = ssim_launch_image<9>(a, b, n, channels, h, w, p, vec, g, c1, c2, ssim_rows, mse_rows, rowq, s); break;
    default: r = ssim_launch_image<11>(a, b, n, channels, h, w, p, vec, g, c1, c2, ssim_rows, mse_rows, rowq, s); break;
  }
  if (!r && mean) launch_chain_mean(rowq, n, rowq + (size_t)n, mean, "ssim_mean_kernels", s);      // workspace: q [n], then the block partials
  return r;
}

}  // namespace gr
