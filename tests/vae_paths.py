"""Error bounds of the VAE sampling layer (gr_vae_sample_dev / gr_vae_sample_backward_dev) against tests/vae_oracle.py, derived from the
operation chains include/ganrev.h states - not tuned against the device.

u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64); gamma(k, w) = k w / (1 - k w) bounds (1 + w)^k - 1.  FN = 3: exp is taken to be within 3 ulp = 6 v
relative, the limit OpenCL sets for double precision - the figure tests/mixture_paths.py uses (the device library and glibc both document less).
Every fp64 bound is two-sided: the library's distance from the exact value plus the float64 reference's, whose chains are the library's.  The
outputs that are floats are compared with the reference's fp64 value BEFORE its rounding to float (z64, K, gh64), so the rounding counts once:
u (|ref| + fp64 bound), and 2^-150 for a result in the float denormals.

  s        exp(0.5 lv): the product by 0.5 is exact; 6 v relative.
  z        se = s eps: 6 v and one product, gamma(7, v) |se|; the add mu + se one more rounding of at most |mu| + |se|: one side
           gamma(8, v) (|mu| + |s eps|).  Two-sided 2 gamma(8, v) = 16 v = 8 * 2^-52 to first order: the k of the expected shape is 8.
  element  mm one rounding; ss = s s carries s twice and a product, gamma(13, v); a = mm + ss, b = a - 1, d = b - lv one rounding each of at most
           mm + ss, mm + ss + 1, mm + ss + 1 + |lv|; the product by 0.5 is exact.  The ss term passes 13 + 3 roundings, every other term fewer:
           one side gamma(16, v) T, T = 0.5 (mm + ss + 1 + |lv|), the element's absolute terms.
  kl_rows  nd - 1 adds in column order (the first, onto +0.0, is exact), every partial sum at most the row's sum of T: one side
           gamma(nd + 16, v) sum_t T.  Two-sided, then the rounding to float.
  kl       the mean of the rows' fp64 bounds, plus the chain of at most RPB adds in a block, ceil(B / RPB) across blocks and one division:
           gamma(RPB + ceil(B / RPB) + 1, v) mean |K| a side.
  gmu      c = kl_weight / B one rounding, c mu one, the add one, of at most |gz| + |c mu|: one side gamma(3, v) (|gz| + |c mu|).
  glv      t1 = (gz eps) (0.5 s): a product, s (6 v), a product: gamma(8, v) |t1|.  t2 = c (0.5 (s s - 1)): ss gamma(13, v), the subtraction one
           rounding of at most ss + 1, c one, the product one: gamma(16, v) |c| 0.5 (ss + 1).  The add t1 + t2 one more:
           one side gamma(17, v) (|t1| + 0.5 |c| (ss + 1)).
"""
import numpy as np

RPB = 512
MAX_ND = 256
U32, U64 = 2.0 ** -24, 2.0 ** -53
FN = 3                      # ulp of exp: OpenCL's limit for double precision
TINY32 = 2.0 ** -150        # half the smallest float denormal


def gamma(k, w):
    return k * w / (1.0 - k * w)


def blocks(n):
    return -(-n // RPB)


def _as_float(ref64, b):
    return b + U32 * (np.abs(ref64) + b) + TINY32


def z_bound(f, mu):
    """f: vae_oracle.forward's result, mu [B x nd] -> [B x nd], against f["z64"]"""
    b = 2.0 * gamma(2 * FN + 2, U64) * (np.abs(np.asarray(mu, np.float64)) + np.abs(f["se"]))
    return _as_float(f["z64"], b)


def rows_bound64(f):
    nd = f["terms"].shape[1]
    return 2.0 * gamma(nd + 4 * FN + 4, U64) * f["terms"].sum(axis=1)


def kl_rows_bound(f):
    """-> [B], against f["K"]"""
    return _as_float(f["K"], rows_bound64(f))


def kl_bound(f):
    """-> float, against f["kl"]"""
    n = len(f["K"])
    return float(rows_bound64(f).mean()) + 2.0 * gamma(RPB + blocks(n) + 1, U64) * float(np.abs(f["K"]).mean())


def gh_bound(g, gz):
    """g: vae_oracle.backward's result, gz [B x nd] -> [B x 2 nd], against g["gh64"]"""
    gz = np.abs(np.asarray(gz, np.float64))
    bmu = 2.0 * gamma(3, U64) * (gz + np.abs(g["cm"]))
    blv = 2.0 * gamma(4 * FN + 5, U64) * (np.abs(g["t1"]) + 0.5 * abs(g["c"]) * (g["s"] * g["s"] + 1.0))
    return _as_float(g["gh64"], np.concatenate([bmu, blv], axis=1))
