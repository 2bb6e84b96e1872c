"""float64 numpy restatement of the VAE sampling layer (include/ganrev.h states the arithmetic; csrc/vae.hip): the same formulas, one rounding per
operation, in the header's order, the fp64 results rounded to float where the header says so.  numpy's exp stands where the device library's does:
that is the one place the two may differ, and tests/vae_paths.py bounds what follows from it.

h [B x 2 nd] = (mu | logvar), eps / gz [B x nd]; eps None is eps = 0.  Inputs are taken as they come (float32 arrays convert exactly; float64
arrays keep their bits, which the finite-difference test uses)."""
import numpy as np

RPB = 512               # rows per block of the mean's row-order chain


def split(h):
    h = np.asarray(h, np.float64)
    nd = h.shape[1] // 2
    return h[:, :nd], h[:, nd:]


def block_mean(K):
    """per block of 512 consecutive rows the K_i in row order from +0.0, the block partials in block order from +0.0, one division by B"""
    K = np.asarray(K, np.float64)
    total = 0.0
    for lo in range(0, len(K), RPB):
        s = 0.0
        for v in K[lo:lo + RPB]:
            s = s + float(v)
        total = total + s
    return total / float(len(K))


def forward(h, eps=None):
    """-> dict: z, kl_rows (float32, the layer's outputs), kl (float), and the fp64 values before the roundings to float: z64, K [B];
    s, se, terms (per element 0.5 (mu^2 + s^2 + 1 + |lv|), the absolute terms of the element KL) for the bounds"""
    mu, lv = split(h)
    ep = np.zeros_like(mu) if eps is None else np.asarray(eps, np.float64)
    s = np.exp(0.5 * lv)
    se = s * ep
    z64 = mu + se
    mm = mu * mu
    ss = s * s
    a = mm + ss
    b = a - 1.0
    d = b - lv
    k = 0.5 * d
    K = np.zeros(mu.shape[0])
    for t in range(mu.shape[1]):
        K = K + k[:, t]
    return dict(z=z64.astype(np.float32), kl_rows=K.astype(np.float32), kl=block_mean(K), z64=z64, K=K, s=s, se=se,
                terms=0.5 * (mm + ss + 1.0 + np.abs(lv)))


def backward(h, eps, gz, kl_weight):
    """the gradient of recon + kl_weight mean_i KL_i with respect to h, gz = d recon / d z -> dict: gh (float32 [B x 2 nd]) and gh64, the fp64
    values before the rounding; t1, t2 (the two terms of glv), cm (c mu), c"""
    mu, lv = split(h)
    ep = np.zeros_like(mu) if eps is None else np.asarray(eps, np.float64)
    gz = np.asarray(gz, np.float64)
    c = float(kl_weight) / float(mu.shape[0])
    s = np.exp(0.5 * lv)
    cm = c * mu
    gmu = gz + cm
    ge = gz * ep
    hs = 0.5 * s
    t1 = ge * hs
    ss = s * s
    sm = ss - 1.0
    hm = 0.5 * sm
    t2 = c * hm
    glv = t1 + t2
    gh64 = np.concatenate([gmu, glv], axis=1)
    return dict(gh=gh64.astype(np.float32), gh64=gh64, t1=t1, t2=t2, cm=cm, c=c, s=s)


def loss(h, eps, target, kl_weight):
    """a loss to differentiate: recon = 0.5 sum (z - target)^2 on the unrounded z, plus kl_weight times the mean KL -> (loss, gz = z - target)"""
    f = forward(h, eps)
    r = f["z64"] - np.asarray(target, np.float64)
    return 0.5 * float((r * r).sum()) + float(kl_weight) * f["kl"], r
