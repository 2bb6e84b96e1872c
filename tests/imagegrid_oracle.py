"""numpy fp32 twin of gr_image_grid_dev, gr_rows_mean_dev and the grid's 8-bit quantisation (include/ganrev.h states them): plain
slicing in the stated order, every operation one IEEE fp32 operation, so the kernels of csrc/render.hip are compared bit for bit.
The colour step is colorspace_oracle's toRgb; nothing here imports the product package.
"""
import numpy as np

import colorspace_oracle as co

F = np.float32


def geometry(n_tiles, slots, h, w, nrow, padding, margin):
    xmaps = min(nrow, n_tiles)
    ymaps = -(-n_tiles // xmaps)
    th, tw = h + 2 * margin, slots * w + 2 * margin
    return xmaps, ymaps, th, tw, (th + padding) * ymaps, (tw + padding) * xmaps


def tiles(srcs, rows, from_space, margin=0, bg=None, inset=None, inset_rgb=(0, 0, 1)):
    """[n_tiles x Cout x TH x TW]: every pixel inside a tile after colour conversion and decoration, before the display range"""
    srcs = [np.asarray(s, F) for s in srcs]
    slots = len(srcs)
    rows = np.asarray(rows, np.int64).reshape(-1, slots)
    n = len(rows)
    _, c, h, w = srcs[0].shape
    cout = 3 if from_space >= 0 else c
    bg = np.zeros((n, 3), F) if bg is None else np.asarray(bg, F).reshape(n, 3)
    ring = np.asarray(inset_rgb, F)[:cout]
    out = np.empty((n, cout, h + 2 * margin, slots * w + 2 * margin), F)
    out[:] = bg[:, :cout, None, None]
    for s in range(slots):
        use = np.nonzero(rows[:, s] >= 0)[0]
        if not len(use):
            continue
        img = srcs[s][rows[use, s]]
        if from_space >= 0:
            img = co.switch(img, co.SPACES[from_space], "rgb")          # rgb -> rgb is the identity: this is toRgb
        img = np.array(img, F)
        if inset is not None:
            for k, t in enumerate(use):
                if inset[t]:
                    img[k, :, 0, :] = ring[:, None]; img[k, :, h - 1, :] = ring[:, None]
                    img[k, :, :, 0] = ring[:, None]; img[k, :, :, w - 1] = ring[:, None]
        out[use, :, margin:margin + h, margin + s * w:margin + (s + 1) * w] = img
    return out


def image_grid(srcs, rows, nrow, from_space=-1, padding=0, margin=0, bg=None, inset=None, inset_rgb=(0, 0, 1), fill=1.0,
               auto_range=False, lo=0.0, hi=1.0):
    """-> float32 [Cout x GH x GW]"""
    t = tiles(srcs, rows, from_space, margin, bg, inset, inset_rgb)
    n, cout, th, tw = t.shape
    slots = len(srcs)
    h, w = th - 2 * margin, (tw - 2 * margin) // slots
    xmaps, ymaps, _, _, gh, gw = geometry(n, slots, h, w, nrow, padding, margin)
    if auto_range:
        lo = F(np.fmin.reduce(t.ravel())) + F(0)                        # compare-selects: a NaN never wins; + 0 makes a zero bound +0
        hi = F(np.fmax.reduce(t.ravel())) + F(0)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        c = np.where(t < lo, lo, t)
        c = np.where(c > hi, hi, c)
        shown = (c - lo) / (hi - lo) if hi != lo else np.zeros_like(t)
    shown = shown.astype(F)
    grid = np.full((cout, gh, gw), F(fill), F)
    for k in range(n):
        y0 = (k // xmaps) * (th + padding) + padding // 2
        x0 = (k % xmaps) * (tw + padding) + padding // 2
        grid[:, y0:y0 + th, x0:x0 + tw] = shown[k]
    return grid


def quantise(grid):
    """[Cout x GH x GW] float32 -> uint8 [GH x GW x Cout]: min(255, max(0, trunc(v * 255 + 0.5))), the product and the sum each rounded"""
    with np.errstate(all="ignore"):
        q = np.asarray(grid, F) * F(255) + F(0.5)
        q = np.where(q > F(255), F(255), q)
        q = np.where(q > F(0), q, F(0))
    return np.ascontiguousarray(q.astype(np.int32).astype(np.uint8).transpose(1, 2, 0))


def rows_mean(table, rows):
    """sequential fp32 sum from zero in list order, one division; zeros for an empty list"""
    table = np.asarray(table, F)
    acc = np.zeros(table.shape[1:], F)
    for r in rows:
        acc = acc + table[int(r)]
    return (acc / F(len(rows))).astype(F) if len(rows) else acc
