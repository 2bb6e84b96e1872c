#!/usr/bin/env python3
"""What ganrev.train --progress costs next to the training it watches: one progress call (progress.TrainPictures.visualize: G over the
100 VIS_NOISE_INPUTS, D over the ranked copy, four gr_progress_grid_dev grids, four PNG files) against one epoch of 30 batches of the same
adversarial.DeviceGame, and against the host route tests/test_gpu_progress.py rebuilds the pictures by (pull_params, host mirrors in
evaluate(), forwardBatched, predictionOrder, the numpy grid of tests/progress_oracle.py, the same four PNG files).  Same process, same
box, batch 32, at ganrev.train's default 1x32x32 (gray) and at 3x64x64 (yuv).  Event-timed on the context's stream (the events see the
host work between two launches too, as wall time), median [min, max] of 30 after one discarded warm-up; the device route is timed first
and again last, so a drift over the run shows.  One more, untimed, progress call runs under gr_set_timing(2) for the kernel-time
breakdown.   python tools/bench_progress.py [out.json]"""
import json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gan-reverser_amd"), os.path.join(ROOT, "tests"), ROOT]
import numpy as np
import ganrev._lib as L
from ganrev import adversarial, models, nn_utils, png, progress
from ganrev.synth import synthetic_images
import progress_oracle as po

ctx = L.default_context(); ctx.set_conv_mode("f16x3")
res = {"device": ctx.info(), "reps": 30, "batch": 32, "epoch_batches": 30, "cases": []}
REPS, B, N_EPOCH, ND = 30, 32, 30, 100


def timed(fn):
    fn()                                                       # the warm-up, discarded
    for i in range(REPS):
        ctx.event_record(2 * i); fn(); ctx.event_record(2 * i + 1)
    ctx.synchronize()
    ms = sorted(ctx.event_elapsed_ms(2 * i, 2 * i + 1) for i in range(REPS))
    return {"ms_median": round(ms[REPS // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def host_route(env, pictures, TRAIN_DATA, epoch, save):
    """the content test's route on the game's own modules: parameters pulled, evaluate(), host forwards, numpy grids, PNG files"""
    G, D, OPT, dims = env.MODEL_G, env.MODEL_D, env.OPT, env.IMG_DIMENSIONS
    G.pull_params(); D.pull_params()
    G.evaluate(); D.evaluate()
    images = nn_utils.forwardBatched(G, pictures.vis_noise_inputs, OPT.batchSize)
    clone = images.copy()
    clone[98], clone[99] = TRAIN_DATA[0], progress.sanity_image(dims, OPT.seed, epoch)
    preds = nn_utils.forwardBatched(D, clone, OPT.batchSize).reshape(100, -1)[:, 0]
    good, bad = nn_utils.predictionOrder(preds, False, 50), nn_utils.predictionOrder(preds, True, 50)
    fs = pictures.from_space
    to_rgb = lambda t: t if fs == L.GR_CS_RGB else ctx.colorspace(t, fs, L.GR_CS_RGB)
    for kind, table, rows, gh, gw in (("images", images, np.arange(100), 10, 10), ("images_good", clone, good, 7, 7),
                                      ("images_bad", clone, bad, 7, 7), ("images_train", TRAIN_DATA[:50], np.arange(50), 8, 7)):
        path = progress.epoch_picture_path(save, kind, 0, epoch)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        png.write_png(path, po.quantise(po.progress_grid(table, rows, len(rows), gh, gw, epoch, fs, to_rgb)))
    G.training(); D.training()


for dims, cs in (((1, 32, 32), "gray"), ((3, 64, 64), "yuv")):
    G, D = models.create_G(dims, ND, True, 2), models.create_D(dims, True, 1)
    env = adversarial.make_env(G, D, dims, batchSize=B, N_epoch=N_EPOCH, noiseDim=ND)
    game = adversarial.DeviceGame(env)
    TRAIN_DATA = synthetic_images(N_EPOCH * B // 2, dims, 7)
    save = tempfile.mkdtemp(prefix="bench_progress_")
    pictures = progress.TrainPictures(game, dims, cs, save, start=0)

    def epoch():
        for b in range(N_EPOCH):
            game.batch(TRAIN_DATA[b * (B // 2):(b + 1) * (B // 2)])

    row = {"dims": list(dims), "colorSpace": cs}
    row["progress_call_device"] = timed(lambda: pictures.visualize(TRAIN_DATA, 7))
    row["epoch_of_30_batches"] = timed(epoch)
    row["progress_call_device_again"] = timed(lambda: pictures.visualize(TRAIN_DATA, 7))
    ctx.synchronize()
    ctx.set_timing(2)
    pictures.visualize(TRAIN_DATA, 7)
    ctx.synchronize()
    kt = [k for k in ctx.kernel_times() if k.get("launches")]
    ctx.set_timing(0)
    row["progress_call_kernels"] = sorted(({"kernel": k["kernel"], "launches": k["launches"], "total_ms": round(k.get("total_ms", 0.0), 4)} for k in kt),
                                          key=lambda k: -k.get("total_ms", 0.0))[:12]
    row["progress_call_kernel_ms"] = round(sum(k.get("total_ms", 0.0) for k in kt), 4)
    row["progress_call_launches"] = int(sum(k["launches"] for k in kt))
    row["progress_call_host"] = timed(lambda: host_route(env, pictures, TRAIN_DATA, 7, save))      # last: it uploads the host vectors again
    d, h, e = (row[k]["ms_median"] for k in ("progress_call_device", "progress_call_host", "epoch_of_30_batches"))
    row["host_over_device"], row["device_call_share_of_epoch"] = round(h / d, 2), round(d / e, 3)
    res["cases"].append(row)
    print(json.dumps(row), flush=True)
    pictures.close(); game.close()

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_progress.json")
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", path)
