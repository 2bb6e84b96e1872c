#!/usr/bin/env python3
"""gr_dataset_images_dev (dataset.lua:149-153 as one fused launch: bytes -> / 255 -> image.scale -> rgbToColorSpace) against
gr_copy2d_dev moving the same number of bytes in the same process, event-timed on the context's stream: median [min, max] of 30
warmed-up launches and achieved bytes/s, for 10 000 rgb images 64x64 -> 32x32 (the reference's sizes, dataset.lua:13-17), 64x64 -> 64x64
(the copy branch), 32x32 -> 64x64 (up-scaling) and 64x64 -> 32x32 from RGBA bytes and into hsl.  Then ganrev.dataset on a folder of
2 000 PNG files of 64x64 written here: host decoding, upload and the launch, in images/s, and the launch's share of that wall time.
    python tools/bench_dataset.py [out.json]"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import dataset as DATASET, png
from ganrev.synth import synthetic_images

ctx = L.default_context()
res = {"device": ctx.info(), "kernel": [], "loader": {}}
WARM, REPS = 10, 30
PL = {"rgb": 3, "y": 1, "yuv": 3, "hsl": 3}


def timed(fn):
    for _ in range(WARM):
        fn()
    for i in range(REPS):
        ctx.event_record(2 * i); fn(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    ms = sorted(ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS))
    return ms[REPS // 2], ms[0], ms[-1]


N = 10000
for (sh, sw, sc, dh, dw, to) in ((64, 64, 3, 32, 32, "rgb"), (64, 64, 3, 64, 64, "rgb"), (32, 32, 3, 64, 64, "rgb"), (64, 64, 4, 32, 32, "rgb"),
                                 (64, 64, 3, 32, 32, "hsl")):
    u8 = np.random.default_rng(1).integers(0, 256, (N, sh, sw, sc), dtype=np.uint8)
    nbytes = u8.size + 4 * N * PL[to] * dh * dw
    src, dst = ctx.upload(u8), ctx.malloc(4 * N * PL[to] * dh * dw)
    med, lo, hi = timed(lambda: ctx.dataset_images_dev(src, N, sh, sw, sc, dh, dw, L.COLOR_SPACES[to], False, dst))
    floats = nbytes // 8                                       # a copy reads and writes: half the bytes each way
    a, b = ctx.malloc(4 * floats), ctx.malloc(4 * floats)
    cmed, clo, chi = timed(lambda: ctx.copy2d(b, floats, a, floats, 1, floats))
    row = {"source": [N, sh, sw, sc], "target": [N, PL[to], dh, dw], "to": to, "bytes": nbytes, "ms_median": round(med, 5), "ms_min": round(lo, 5),
           "ms_max": round(hi, 5), "GBps": round(nbytes / med / 1e6, 1), "copy_ms_median": round(cmed, 5), "copy_ms_min": round(clo, 5),
           "copy_ms_max": round(chi, 5), "copy_GBps": round(nbytes / cmed / 1e6, 1), "ratio_to_copy": round(cmed / med, 3)}
    res["kernel"].append(row)
    print(f"{sh}x{sw}x{sc} -> {to} {dh}x{dw}, {N} images: {med * 1e3:.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}] {row['GBps']} GB/s; copy of {nbytes} B: "
          f"{cmed * 1e3:.1f} us [{clo * 1e3:.1f}, {chi * 1e3:.1f}] {row['copy_GBps']} GB/s", flush=True)
    for p in (src, dst, a, b):
        ctx.free(p)

NF = 2000
with tempfile.TemporaryDirectory() as d:
    imgs = (synthetic_images(NF, (3, 64, 64), 2).transpose(0, 2, 3, 1) * 255).astype(np.uint8)
    for i in range(NF):
        png.write_png(os.path.join(d, "%05d.png" % i), imgs[i])
    DATASET.setDirs([d]); DATASET.setFileExtension("png"); DATASET.setColorSpace("rgb"); DATASET.setHeight(32); DATASET.setWidth(32)
    DATASET.loadImages(1, 64).free()                           # warm-up: code object, allocator
    t0 = time.perf_counter()
    for p in DATASET.paths:
        DATASET.decode(p)
    t_decode = time.perf_counter() - t0
    ctx.set_timing(2)
    t0 = time.perf_counter()
    r = DATASET.loadImages(1, NF); ctx.synchronize()
    t_load = time.perf_counter() - t0
    kt = ctx.kernel_times(); ctx.set_timing(0)
    r.free()
k_ms = sum(k["total_ms"] for k in kt if k["kernel"].startswith("dataset_images_kernel"))
res["loader"] = {"files": NF, "format": "png 64x64x3 (ganrev.png, pure Python inflate + unfilter)", "target": [32, 32], "load_s": round(t_load, 4),
                 "images_per_s": round(NF / t_load, 1), "host_decode_s": round(t_decode, 4), "kernel_ms": round(k_ms, 5),
                 "kernel_launches": sum(k["launches"] for k in kt if k["kernel"].startswith("dataset_images_kernel")),
                 "kernel_share_of_load": round(k_ms / 1e3 / t_load, 6), "decode_share_of_load": round(t_decode / t_load, 4)}
print(f"loader: {NF} PNG files in {t_load:.3f} s = {NF / t_load:.0f} images/s; host decoding alone {t_decode:.3f} s; the kernel {k_ms * 1e3:.1f} us = "
      f"{100 * k_ms / 1e3 / t_load:.4f} % of the load", flush=True)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_dataset.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
