"""Mirror of the reference's train.lua main loop (train.lua:125-257): build or load G and D, then per epoch load N_epoch *
batchSize / 2 * D_iterations training images (train.lua:214-216), play adversarial.train on them and save
{D, G, opt, epoch} as a Torch7 checkpoint (train.lua:241-257) - the file train_r.lua:68 and apply_r.lua:62 read G from.
Without --network, G starts from <G_pretrained_dir>/g_pretrained_CxHxW_ndN.net (ganrev.pretrain_g) when that file exists and
--nopretraining is not given (train.lua:148-161).

    python -m ganrev.train --epochs 5 --N_epoch 30 --batchSize 32 --save logs [--dataset DIR [--cacheDataset] | --data images.npy] [--compat]

Same option names and defaults as train.lua:12-60 for what is mirrored.  Normalisation and the `display` UI are out of scope (SURVEY.md
section 2).  --progress writes visualizeProgress's pictures (train.lua:268-319) per epoch -
<save>/images, images_good, images_bad, images_train - and <save>/plot_data.json from the device-resident models (ganrev.progress),
and stores vis_noise_inputs and plot_data in the checkpoint, which --network reuses (train.lua:116,204,256); the trained parameters are
bit for bit those of a run without it.  It needs the fast loop (refused with --compat).  Training images come from --dataset DIR (ganrev.dataset = dataset.lua: DATASET.loadRandomImages per
epoch, train.lua:216; files matching --fileExtension), from --data (an [N x C x H x W] float32 .npy in [0, 1]) or, without either,
from a synthetic generator.  --colorSpace takes the
reference's rgb | yuv | hsl | y (train.lua:45) besides gray (= y, one channel): three-channel rgb images are converted with
nn_utils.rgbToColorSpace once per epoch load.

Two loops, as in ganrev.train_r:
  fast (default)  - adversarial.DeviceGame: every batch device-resident, parameters pulled to the host only before a save;
  --compat        - adversarial.train, the closures exactly as adversarial.lua:66-133 spells them.
"""
import argparse
import os
import time

import numpy as np

from . import _lib as L
from . import adversarial, models, nn_utils, pretrain_g, progress, scripts, t7
from .synth import synthetic_images          # also the name tests and tools import it by: train.synthetic_images


def parse(argv=None):
    p = argparse.ArgumentParser(description="train.lua options (train.lua:12-60)")
    p.add_argument("--save", default="logs")                       # train.lua:13
    p.add_argument("--saveFreq", type=int, default=30)             # train.lua:14
    p.add_argument("--network", default="")                        # train.lua:15: continue from this checkpoint
    p.add_argument("--G_pretrained_dir", default="logs")            # train.lua:20: where pretrain_g.lua saved G
    p.add_argument("--nopretraining", action="store_true")          # train.lua:21
    p.add_argument("--batchSize", type=int, default=32)
    p.add_argument("--N_epoch", type=int, default=30)
    p.add_argument("--epochs", type=int, default=1, help="epochs to play (train.lua runs until interrupted)")
    p.add_argument("--G_L1", type=float, default=0.0)
    p.add_argument("--G_L2", type=float, default=0.0)
    p.add_argument("--D_L1", type=float, default=0.0)
    p.add_argument("--D_L2", type=float, default=1e-4)
    p.add_argument("--D_iterations", type=int, default=1)
    p.add_argument("--G_iterations", type=int, default=1)
    p.add_argument("--D_clamp", type=float, default=1.0)
    p.add_argument("--G_clamp", type=float, default=5.0)
    p.add_argument("--D_optmethod", default="adam", help="sgd|adagrad|adadelta|adamax|adam|rmsprop, each a fused device update (train.lua:37)")
    p.add_argument("--G_optmethod", default="adam")
    p.add_argument("--D_sgd_lr", type=float, default=0.02)
    p.add_argument("--G_sgd_lr", type=float, default=0.02)
    p.add_argument("--D_sgd_momentum", type=float, default=0.0)
    p.add_argument("--G_sgd_momentum", type=float, default=0.0)
    p.add_argument("--G_model", default="create_G3", choices=["create_G3", "create_G4"],
                   help="the constructor of a fresh G: models.create_G3 (what models.create_G returns) or the 32-branch models.create_G4 (32x32 only)")
    p.add_argument("--noiseDim", type=int, default=100)
    p.add_argument("--noiseMethod", default="normal", choices=["normal", "uniform"])
    p.add_argument("--height", type=int, default=32)
    p.add_argument("--width", type=int, default=32)
    p.add_argument("--colorSpace", default="gray", choices=["gray", "rgb", "y", "yuv", "hsl"])      # train.lua:45 rgb|yuv|hsl|y; gray = y
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--data", default="", help="[N x C x H x W] float32 .npy of training images; default: synthetic")
    scripts.add_dataset_options(p)                                   # train.lua:16 --dataset
    p.add_argument("--compat", action="store_true")
    scripts.add_progress_option(p)
    p.add_argument("--conv-mode", default="f16x3", choices=["f32", "bf16x6", "f16x3"])
    p.add_argument("--quiet", action="store_true")
    return p.parse_args(argv)


def pretrained_G_path(OPT, dims):
    """train.lua:148-149: <G_pretrained_dir>/g_pretrained_CxHxW_ndN.net when it exists and --nopretraining is not given, else None"""
    path = os.path.join(OPT.G_pretrained_dir, pretrain_g.checkpoint_name(dims, OPT.noiseDim))
    return path if not OPT.nopretraining and os.path.isfile(path) else None


def create_or_load_G(OPT, dims):
    """train.lua:148-161: pretrain_g.lua's decoder in training mode, or a fresh create_G; --G_model create_G4 builds models.create_G4
    instead (always fresh: pretrain_g trains create_G's decoder only)"""
    if OPT.G_model == "create_G4":
        return models.create_G4(dims, OPT.noiseDim, True, OPT.seed + 1)
    path = pretrained_G_path(OPT, dims)
    if path is None:
        if not OPT.quiet:
            print("<trainer> Note: Did not find pretrained G")
        return models.create_G(dims, OPT.noiseDim, True, OPT.seed + 1)
    if not OPT.quiet:
        print("<trainer> loading pretrained G...")
    return scripts.load_checkpoint(path)["G"].training()


def save(OPT, env, epoch, quiet=True, pictures=None):
    """train.lua:236-257: logs/adversarial.net (the previous file moved to .old), {D, G, opt, epoch}; with --progress (pictures)
    also {plot_data, vis_noise_inputs}, as train.lua:256."""
    filename = os.path.join(OPT.save, "adversarial.net")
    env.MODEL_G.pull_params(); env.MODEL_D.pull_params()             # current BatchNorm running statistics (and parameters) into the modules
    os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
    if os.path.isfile(filename):
        os.replace(filename, filename + ".old")
    if not quiet:
        print("<trainer> saving network to %s" % filename)
    extra = {} if pictures is None else dict(plot_data=pictures.plot_data, vis_noise_inputs=pictures.vis_noise_inputs)
    t7.save_checkpoint(filename, D=env.MODEL_D, G=env.MODEL_G, opt=scripts.opt_table(OPT), epoch=epoch, **extra)
    return filename


def main(argv=None):
    OPT = parse(argv)
    scripts.refuse_progress_in_compat(OPT)
    dims = scripts.image_dims(OPT.colorSpace, OPT.height, OPT.width)
    if OPT.G_model == "create_G4" and not OPT.network and (OPT.height, OPT.width) != (32, 32):
        # models.lua:152-153 computes a start size and never uses it: the branches are 16x16 -> 32x32 whatever the options say
        raise SystemExit("--G_model create_G4 paints 32x32 images only (models.lua:157-183): got --height %d --width %d" % (OPT.height, OPT.width))
    ctx = L.default_context()
    ctx.set_conv_mode(OPT.conv_mode)
    epoch0, ck = 1, {}
    if OPT.network:                                                   # train.lua:125-140
        ck = scripts.load_checkpoint(OPT.network)
        MODEL_D, MODEL_G, epoch0 = ck["D"], ck["G"], int(ck.get("epoch", 0)) + 1      # train.lua:113  EPOCH = tmp.epoch + 1
    else:                                                             # train.lua:143,160
        MODEL_D = models.create_D(dims, True, OPT.seed)
        MODEL_G = create_or_load_G(OPT, dims)
    env = adversarial.make_env(MODEL_G, MODEL_D, dims, **{k: getattr(OPT, k) for k in
                               ("batchSize", "N_epoch", "noiseDim", "noiseMethod", "G_L1", "G_L2", "D_L1", "D_L2", "D_iterations", "G_iterations",
                                "D_clamp", "G_clamp", "D_optmethod", "G_optmethod", "seed", "D_sgd_lr", "G_sgd_lr", "D_sgd_momentum", "G_sgd_momentum")})
    env.EPOCH = epoch0
    data = np.load(OPT.data).astype(np.float32) if OPT.data else None
    DATASET = scripts.open_dataset(OPT, OPT.colorSpace, OPT.height, OPT.width, ctx)      # train.lua:81-85; --cacheDataset: every file decoded here, once
    game = None if OPT.compat else adversarial.DeviceGame(env)       # every method of train.lua:37-38 has its fused device update
    pictures = None
    if OPT.progress:                                                  # train.lua:116,203-204: VIS_NOISE_INPUTS of the checkpoint, or fresh
        vis, plot = ck.get("vis_noise_inputs"), ck.get("plot_data")
        pictures = progress.TrainPictures(game, dims, OPT.colorSpace, OPT.save, vis_noise_inputs=vis if isinstance(vis, np.ndarray) else None,
                                          plot_data=plot if isinstance(plot, list) else None)
    N_epoch = OPT.N_epoch if OPT.N_epoch > 0 else 100                 # adversarial.lua:42-45: N_epoch <= 0 means 100 batches
    D_it, G_it = max(0, OPT.D_iterations), max(0, OPT.G_iterations)   # 0 iterations freeze that net (adversarial.lua:127,168 loop zero times)
    # a continued run must not replay the first epochs' noise: the counters start where epoch0 - 1 finished epochs left them
    # (the reference's Torch RNG is not restored from a checkpoint either; the optimiser state restarts empty, as train.lua does)
    done = (epoch0 - 1) * N_epoch * (D_it + G_it)
    env.noise_counter = getattr(env, "noise_counter", 0) + done
    if game is not None:
        game.noise_counter += done
    # train.lua:214 multiplies OPT.N_epoch itself; with N_epoch <= 0 that loads nothing while adversarial.lua:42-45 still runs 100
    # batches and indexes past the loaded examples - here the 100 batches get their images
    nbLoad = (N_epoch * OPT.batchSize // 2) * D_it
    cursor, last, t0, images = (epoch0 - 1) * nbLoad, None, time.perf_counter(), 0
    TRAIN_DATA = None
    for _ in range(OPT.epochs):
        if isinstance(TRAIN_DATA, nn_utils.DeviceTensor):
            TRAIN_DATA.free()                                         # the last epoch's draw from the cache
        if DATASET is not None:
            TRAIN_DATA = scripts.load_random_images(DATASET, nbLoad)   # train.lua:216; already in --colorSpace (dataset.lua:153); --cacheDataset: a device table
        elif data is not None:
            idx = (cursor + np.arange(nbLoad)) % len(data); cursor += nbLoad
            TRAIN_DATA = data[idx]
        else:
            TRAIN_DATA = synthetic_images(nbLoad, dims, OPT.seed * 7919 + env.EPOCH * 3)
        if DATASET is None and scripts.needs_conversion(TRAIN_DATA, OPT.colorSpace):
            # rgb images seen in another space (dataset.lua:153): one gr_colorspace_host call per epoch load
            TRAIN_DATA = nn_utils.rgbToColorSpace(np.ascontiguousarray(TRAIN_DATA, np.float32), OPT.colorSpace)
        if pictures is not None:
            pictures.visualize(TRAIN_DATA, env.EPOCH)                 # train.lua:222-224, between the load and the epoch
        if game is None:
            adversarial.train(env, TRAIN_DATA, quiet=OPT.quiet)       # train.lua:229
            last = (env.last_losses["D"][-1], env.last_losses["G"][-1])
        else:
            per = (OPT.batchSize // 2) * D_it                         # real images one batch consumes: batchSize/2 per D iteration (adversarial.lua:139-149)
            for b in range(N_epoch):
                want = b == N_epoch - 1
                on_device = isinstance(TRAIN_DATA, nn_utils.DeviceTensor)
                res = game.batch(TRAIN_DATA.rows(b * per, (b + 1) * per) if on_device else TRAIN_DATA[b * per:(b + 1) * per], want_loss=want)
                if want:
                    last = res
        images += N_epoch * OPT.batchSize * G_it
        if not OPT.quiet:
            print("<trainer> epoch %d: loss D=%.4f G=%.4f" % (env.EPOCH, last[0], last[1]))
        if pictures is not None:
            pictures.log(env.EPOCH, last[0], last[1])
        if env.EPOCH % OPT.saveFreq == 0:                             # train.lua:232-234
            if game is not None:
                game.sync_to_host()
            save(OPT, env, env.EPOCH, OPT.quiet, pictures)
        env.EPOCH += 1
    if game is not None:
        game.sync_to_host()
    if isinstance(TRAIN_DATA, nn_utils.DeviceTensor):
        TRAIN_DATA.free()
    path = save(OPT, env, env.EPOCH - 1, OPT.quiet, pictures)         # train.lua:209-211 "Last epoch reached."
    if pictures is not None:
        pictures.close()
    if not OPT.quiet:
        print("<trainer> %.1f generated images/s" % (images / (time.perf_counter() - t0)))
    return dict(path=path, last_losses=last, epoch=env.EPOCH - 1, env=env, pictures=pictures)


if __name__ == "__main__":
    main()
