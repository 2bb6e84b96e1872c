#!/usr/bin/env python3
"""What a --dataset draw costs with and without --cacheDataset, next to the epoch it feeds.  A folder of 64x64 RGB PNG files is written
from synth.synthetic_images (FILES of them); the draw is the one a default ganrev.train epoch makes - scripts.load_random_images of
30 * 32 / 2 = 480 files - to 3x32x32 rgb and to 3x64x64 yuv.

  uncached   decode 480 files, upload the bytes, one dataset_images_kernel launch per size group, download the table (a host array)
  cached     one dataset_gather_kernel launch over the cache (a device table), then a wait for the stream

Wall time (time.perf_counter) around work that ends in a synchronise: the uncached draw ends in its download, the cached draw is followed by
ctx.synchronize() inside the timed window; its table is freed outside it.  The two alternate, draw by draw, in one process after one
discarded warm-up each; median [min, max] of REPS.  The uncached loader is the code the parent commit has: its figure is the parent's cost.
The uncached draw leaves a host array that the loops upload again batch by batch; that upload is NOT in its figure.  One more, untimed,
draw of each kind runs under gr_set_timing(2) for the kernel times.  DATASET.cache() on that folder is timed the same way (BUILD_REPS), and one
30-batch epoch of adversarial.DeviceGame at the same shapes (batch 32, event-timed as tools/bench_progress.py does) is the yardstick.
   python tools/bench_dataset_cache.py [out.json]"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import adversarial, dataset as DATASET, models, nn_utils, png, scripts
from ganrev.synth import synthetic_images

REPS, BUILD_REPS, B, N_EPOCH, ND, FILES, DRAW = 30, 30, 32, 30, 100, 2048, 480
ctx = L.default_context(); ctx.set_conv_mode("f16x3")
res = {"device": ctx.info(), "reps": REPS, "build_reps": BUILD_REPS, "files": FILES, "draw": DRAW, "source": [64, 64, 3], "batch": B, "epoch_batches": N_EPOCH,
       "cases": []}


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def event_timed(fn):
    fn()                                                       # the warm-up, discarded
    for i in range(REPS):
        ctx.event_record(2 * i); fn(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    return stats(ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS))


def kernels(fn):
    ctx.synchronize(); ctx.set_timing(2)
    fn(); ctx.synchronize()
    kt = [k for k in ctx.kernel_times() if k.get("launches") and k["kernel"].startswith("dataset_")]
    ctx.set_timing(0)
    return [{"kernel": k["kernel"], "launches": k["launches"], "total_ms": round(k.get("total_ms", 0.0), 4)} for k in kt]


folder = tempfile.mkdtemp(prefix="bench_dataset_cache_")
faces = synthetic_images(FILES, (3, 64, 64), 5)
for i in range(FILES):
    png.write_png(os.path.join(folder, "face_%05d.png" % i), np.ascontiguousarray((faces[i].transpose(1, 2, 0) * 255 + 0.5).astype(np.uint8)))
DATASET.setDirs([folder]); DATASET.setFileExtension("png"); DATASET.setSeed(1)

DATASET.cache(ctx)                                             # the warm-up, discarded
build = []
for _ in range(BUILD_REPS):
    DATASET.uncache()
    build.append(wall(lambda: (DATASET.cache(ctx), ctx.synchronize()))[0])
res["cache_build"] = dict(stats(build), bytes=DATASET._cache.size()[1])
print(json.dumps(res["cache_build"]), flush=True)
held = DATASET._cache


def uncached_draw():
    DATASET._cache = None                                      # the loader as it is without the option (the cache stays where it is)
    try:
        return scripts.load_random_images(DATASET, DRAW)
    finally:
        DATASET._cache = held


def cached_draw():
    table = scripts.load_random_images(DATASET, DRAW)
    ctx.synchronize()
    return table


for dims, cs in (((3, 32, 32), "rgb"), ((3, 64, 64), "yuv")):
    DATASET.setColorSpace(cs); DATASET.setHeight(dims[1]); DATASET.setWidth(dims[2])
    uncached_draw(); cached_draw().free()                      # the warm-up of both, discarded
    DATASET.setSeed(1); want = uncached_draw()
    DATASET.setSeed(1); got = cached_draw()
    assert np.array_equal(want.view(np.uint32), got.numpy().view(np.uint32)), "the cached draw is not the uncached draw"
    got.free()
    plain, cached = [], []
    for _ in range(REPS):                                      # alternating: a drift of the box shows in both
        plain.append(wall(uncached_draw)[0])
        ms, table = wall(cached_draw)
        cached.append(ms); table.free()
    row = {"dims": list(dims), "colorSpace": cs, "uncached_draw": stats(plain), "cached_draw": stats(cached)}
    row["uncached_over_cached"] = round(row["uncached_draw"]["ms_median"] / row["cached_draw"]["ms_median"], 1)
    row["ranges_overlap"] = bool(row["cached_draw"]["ms_max"] >= row["uncached_draw"]["ms_min"])
    row["uncached_kernels"] = kernels(uncached_draw)
    row["cached_kernels"] = kernels(lambda: cached_draw().free())
    G, D = models.create_G(dims, ND, True, 2), models.create_D(dims, True, 1)
    game = adversarial.DeviceGame(adversarial.make_env(G, D, dims, batchSize=B, N_epoch=N_EPOCH, noiseDim=ND))
    TRAIN_DATA = synthetic_images(N_EPOCH * B // 2, dims, 7)
    row["epoch_of_30_batches"] = event_timed(lambda: [game.batch(TRAIN_DATA[b * (B // 2):(b + 1) * (B // 2)]) for b in range(N_EPOCH)])
    e = row["epoch_of_30_batches"]["ms_median"]
    row["uncached_draw_share_of_epoch"] = round(row["uncached_draw"]["ms_median"] / e, 3)
    row["cached_draw_share_of_epoch"] = round(row["cached_draw"]["ms_median"] / e, 4)
    res["cases"].append(row)
    print(json.dumps(row), flush=True)
    game.close()
DATASET.uncache()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_dataset_cache.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
