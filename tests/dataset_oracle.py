"""numpy oracle of dataset.lua's per-image work as include/ganrev.h states it for gr_image_scale_* and gr_dataset_images_dev:
image.scale in its default bilinear mode (two passes of scaleLinear_rowcol, rows first), the bytes / 255 in front of it and
rgbToColorSpace / NN_UTILS.normalize behind it.

The scale pass is written once, as scalar loops over the output index and the source taps, one IEEE operation per line.  The value
arithmetic runs in `dtype`: float32 gives the bit-exact twin of the kernels, float64 the yardstick the twin itself is held to.  The
indices and fractional weights (i, f) are DEFINED by the fp32 operations of the header in both cases - they are the filter, not part
of its rounding error - so the float64 evaluation applies exactly the same taps with exactly the same weights.

Lines are the last axis of an array; every leading element is an independent line that goes through the same scalar steps."""
import numpy as np

import colorspace_oracle as co

F = np.float32
MAX_LEN = 32768          # include/ganrev.h: the largest side


def taps(src_len, dst_len):
    """The filter of one pass: for every output index the list of (source index, fp32 weight or None for 1) and the fp32 parts n is summed
    from (None: no division).  Exactly the header's fp32 steps for i and f."""
    assert 1 <= src_len <= MAX_LEN and 1 <= dst_len <= MAX_LEN
    out = []
    if dst_len == src_len:
        return [("copy", di) for di in range(dst_len)]
    if dst_len > src_len:
        if src_len == 1:
            return [("copy", 0) for _ in range(dst_len)]
        scale = F(F(src_len - 1) / F(dst_len - 1))
        for di in range(dst_len - 1):
            f = F(F(di) * scale)
            i = int(f)
            f = F(f - F(i))
            assert 0 <= i and i + 1 < src_len, (src_len, dst_len, di, i)
            out.append(("lerp", i, f))
        out.append(("copy", src_len - 1))
        return out
    scale = F(F(src_len) / F(dst_len))
    i0, f0 = 0, F(0)
    for di in range(dst_len):
        f1 = F(F(di + 1) * scale)
        i1 = int(f1)
        f1 = F(f1 - F(i1))
        assert 0 <= i0 < src_len and i1 <= src_len, (src_len, dst_len, di, i0, i1)
        out.append(("box", i0, f0, i1, f1))
        i0, f0 = i1, f1
    return out


def scale_lines(src, dst_len, dtype=np.float32):
    """scaleLinear_rowcol(src_len, dst_len) on every line (last axis) of src"""
    t = np.dtype(dtype).type
    src = np.asarray(src, dtype)
    src_len = src.shape[-1]
    dst = np.empty(src.shape[:-1] + (dst_len,), dtype)
    one = t(1)
    for di, tap in enumerate(taps(src_len, dst_len)):
        if tap[0] == "copy":
            dst[..., di] = src[..., tap[1]]
        elif tap[0] == "lerp":
            _, i, f = tap
            f = t(f)
            w = one - f
            a = w * src[..., i]
            b = f * src[..., i + 1]
            dst[..., di] = a + b
        else:
            _, i0, f0, i1, f1 = tap
            f0, f1 = t(f0), t(f1)
            n = one - f0
            acc = n * src[..., i0]
            for s in range(i0 + 1, i1):
                acc = acc + src[..., s]
                n = n + one
            if i1 < src_len:
                p = f1 * src[..., i1]
                acc = acc + p
                n = n + f1
            dst[..., di] = acc / n
    assert dst.dtype == np.dtype(dtype)
    return dst


def scale(images, dh, dw, dtype=np.float32):
    """image.scale(src, dw, dh) on [... x sh x sw]: the row pass (sw -> dw, rounded to `dtype`), then the column pass (sh -> dh)"""
    rows = scale_lines(images, dw, dtype)
    cols = scale_lines(np.swapaxes(rows, -1, -2), dh, dtype)
    return np.ascontiguousarray(np.swapaxes(cols, -1, -2))


def roundings(src_len, dst_len):
    """fp32 roundings on the longest value path of one pass (tests/test_dataset_host.py derives the bound from it)"""
    if dst_len == src_len or src_len == 1:
        return 0
    if dst_len > src_len:
        return 4                                              # 1 - f, two products, one sum
    most = 0
    for _, i0, f0, i1, f1 in taps(src_len, dst_len):
        mid = max(0, i1 - i0 - 1)
        last = 1 if i1 < src_len else 0
        # 1 - f0; its product; per middle tap one sum into acc and one into n; the last tap's product and two sums; the division
        most = max(most, 2 + 2 * mid + 3 * last + 1)
    return most


def bytes_to_planar(u8, dtype=np.float32):
    """image.load(fp, 3, "float") from decoded bytes [n x h x w x sc]: / 255, grey replicated, alpha dropped -> [n x 3 x h x w]"""
    t = np.dtype(dtype).type
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 4 and u8.shape[3] in (1, 3, 4), (u8.dtype, u8.shape)
    v = u8.astype(dtype) / t(255)
    v = np.repeat(v, 3, axis=3) if u8.shape[3] == 1 else v[..., :3]
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2))


def normalize(x):
    """utils/nn_utils.lua:371-375 on a copy: * 2, + (-1), clamp to [-1, 1]"""
    t = x.dtype.type
    v = x * t(2)
    v = v + t(-1)
    v = np.where(v < t(-1), t(-1), v)
    return np.where(v > t(1), t(1), v).astype(x.dtype)


def dataset_images(u8, dh, dw, to, normalise=False, dtype=np.float32):
    """gr_dataset_images_dev: uint8 [n x sh x sw x sc] -> [n x planes(to) x dh x dw]"""
    out = co.from_rgb(scale(bytes_to_planar(u8, dtype), dh, dw, dtype), to, dtype)
    return normalize(out) if normalise else np.ascontiguousarray(out)


def load_files(arrays, dh, dw, to, normalise=False):
    """the loader on decoded files of any sizes, in the order given: [len(arrays) x planes(to) x dh x dw]"""
    return np.concatenate([dataset_images(a[None], dh, dw, to, normalise) for a in arrays], axis=0)
