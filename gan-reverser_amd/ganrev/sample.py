"""Mirror of the reference's sample.lua (sample.lua:9-148): load G and D from a checkpoint, let G create 1024 images, keep the 64
best and the 64 worst according to D and 64 random ones, and with --neighbours find the nearest training image (torch.dist) of
each of the 16 best.

    python -m ganrev.sample --save logs --network adversarial.net --dataset DIR --writeTo samples [--neighbours]

Same option names and defaults as sample.lua:9-24.  The training set comes from --dataset DIR (ganrev.dataset = dataset.lua; files
matching --fileExtension; --neighbours searches the device-resident table DATASET.loadImages leaves, sample.lua:132) or from --data
(an [N x C x H x W] float32 .npy, as in ganrev.train), and each run writes one samples_<run>.npz into --writeTo with best, best_pred,
worst, worst_pred, random and, with --neighbours, neighbour_idx, neighbour_dist and neighbours.  With --render the run's pictures
(sample.lua:96-118: random1024, random256, best, worst, random and best_*_neighbours, named <name>_<run>_base) are written beside it
as PNG - toGrid / toNeighboursGrid (sample.lua:166-185) on the GPU through ganrev.render, display range taken from the picture itself
as image.toDisplayTensor does without min / max.  trainset_s1 (sample.lua:77-83: 64 random training images) is written with --dataset.  Random
choices use numpy's generator seeded by --seed (Torch's generator is not reproduced).
"""
import argparse
import os

import numpy as np

from . import _lib as L
from . import nn_utils, scripts, t7


def parse(argv=None):
    p = argparse.ArgumentParser(description="sample.lua options (sample.lua:9-24)")
    p.add_argument("--save", default="logs")                          # sample.lua:10
    p.add_argument("--network", default="adversarial.net")            # sample.lua:11
    p.add_argument("--neighbours", action="store_true", help="nearest training image of each of the 16 best images")
    p.add_argument("--colorSpace", default="rgb", help="rgb|yuv|hsl|y (y: one channel, else three)")
    p.add_argument("--writeTo", default="samples")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--gpu", type=int, default=0)
    p.add_argument("--runs", type=int, default=1)
    p.add_argument("--noiseDim", type=int, default=32)
    p.add_argument("--noiseMethod", default="normal", choices=["normal", "uniform"])
    p.add_argument("--batchSize", type=int, default=16)
    p.add_argument("--height", type=int, default=32)
    p.add_argument("--width", type=int, default=32)
    scripts.add_dataset_options(p)                                    # sample.lua:19 --dataset
    p.add_argument("--data", default="", help="[N x C x H x W] float32 .npy: the training set --neighbours searches")
    p.add_argument("--render", action="store_true", help="also write the run's image grids as PNG files (ganrev.render)")
    return p.parse_args(argv)


def image_dims(opt):
    return scripts.image_dims(opt.colorSpace, opt.height, opt.width)          # sample.lua:38-42


def loadModels(opt):
    """sample.lua:200-222: G and D of the checkpoint, both in evaluate mode; warns when the checkpoint's opt differs in size or colour space."""
    ck = t7.load_checkpoint(os.path.join(opt.save, opt.network))
    if "_unconverted" in ck:
        raise L.GanrevError(f"{opt.network}: {ck['_unconverted']}")
    G, D = ck["G"], ck["D"]
    G.evaluate()
    D.evaluate()
    fo = ck.get("opt") or {}
    if opt.width != fo.get("width") or opt.height != fo.get("height") or opt.colorSpace != fo.get("colorSpace"):
        print("[WARNING] colorSpace/height/width mismatch. Loaded network: %s/%s/%s, current settings: %s/%d/%d"
              % (fo.get("colorSpace"), fo.get("height"), fo.get("width"), opt.colorSpace, opt.height, opt.width))
    return G, D


def noise_seed(opt, run):
    """seed of createNoiseInputs for run `run` (1-based)"""
    return opt.seed + run - 1


def findClosestNeighboursOf(ctx, images, table_dev, n, d, k=1):
    """sample.lua:130-148 on the GPU: for each image the nearest row(s) of the device-resident training table [n x d] by torch.dist
    -> (idx [m, k], dist [m, k])."""
    return ctx.l2_nearest(None, np.asarray(images, np.float32).reshape(len(images), -1), k, table_dev=table_dev, n=n, d=d)


def toGrid(ctx, images, nrow, colorSpace, path=None):
    """sample.lua:166-168: image.toDisplayTensor{input = toRgb(images), nrow = nrow}, no min / max -> uint8 [GH x GW x 3]; the host
    images are uploaded, the grid is rendered on the GPU"""
    from . import render
    images = np.ascontiguousarray(images, dtype=np.float32)
    with nn_utils.DeviceTensor(ctx, images.shape) as t:
        ctx.upload(images, t.ptr)
        return render.grid(t, np.arange(len(images)), nrow, colorSpace, auto_range=True, path=path)


def main(argv=None):
    opt = parse(argv)
    if opt.gpu < 0:
        raise SystemExit("[ERROR] Sample script currently only runs on GPU")      # sample.lua:26-29
    dims = image_dims(opt)
    ctx = L.default_context()
    G, D = loadModels(opt)
    DATASET = scripts.open_dataset(opt, opt.colorSpace, opt.height, opt.width, ctx)      # sample.lua:46-50; --cacheDataset: both loads below come from the cache
    data = table = None
    if opt.neighbours:
        if DATASET is not None:
            # sample.lua:132 DATASET.loadImages(0, 9999999) - with 1: dataset.lua:100 asserts startAt > 0.  Loaded once, not per call;
            # the table stays where the loader's kernel left it and gr_l2_nearest_dev searches it there.
            table = DATASET.loadImages(1, 9999999).data
        elif opt.data:
            data = np.ascontiguousarray(np.load(opt.data), dtype=np.float32)
        else:
            raise SystemExit("--neighbours needs --dataset or --data (the training set)")
    os.makedirs(opt.writeTo, exist_ok=True)
    rng = np.random.default_rng(opt.seed)
    print("Sampling...")
    written = []
    for run in range(1, opt.runs + 1):
        images = nn_utils.createImages(G, 1024, opt.noiseDim, opt.batchSize, opt.noiseMethod, noise_seed(opt, run))
        if images.shape[1:] != dims:                                  # sample.lua:86-93
            print("[WARNING] dimension mismatch between images generated by base G and command line parameters")
            print("Dimension G:", images.shape[1:])
            print("Settings:", dims)
        best, best_pred = nn_utils.sortImagesByPrediction(D, images, False, 64, opt.batchSize)
        worst, worst_pred = nn_utils.sortImagesByPrediction(D, images, True, 64, opt.batchSize)
        name = lambda what: os.path.join(opt.writeTo, "%s_%04d_base.png" % (what, run))
        if opt.render and DATASET is not None:                        # sample.lua:77-83
            from . import render
            train = DATASET.loadRandomImages(64)
            render.grid(train.images, np.arange(train.size()), 8, opt.colorSpace, auto_range=True, path=name("trainset_s1"))
            train.free()
        if opt.render:                                                # sample.lua:96-97 (drawn before the 64 random ones, as there)
            toGrid(ctx, images[rng.permutation(len(images))[:256]], 16, opt.colorSpace, name("random256"))
            toGrid(ctx, images, 32, opt.colorSpace, name("random1024"))
        random = images[rng.choice(len(images), 64, replace=False)]
        out = dict(best=best, best_pred=best_pred, worst=worst, worst_pred=worst_pred, random=random)
        if opt.render:                                                # sample.lua:107-109
            for what, imgs in (("best", best), ("worst", worst), ("random", random)):
                toGrid(ctx, imgs, 8, opt.colorSpace, name(what))
        if opt.neighbours:                                            # sample.lua:115-123
            shape = data.shape if table is None else table.shape
            n, d = shape[0], int(np.prod(shape[1:]))
            if d != int(np.prod(best.shape[1:])):
                raise SystemExit(f"the training images have {d} values, G's images {int(np.prod(best.shape[1:]))}")
            table_dev = ctx.upload(data) if table is None else table.ptr      # --data: once per run
            try:
                idx, dist = findClosestNeighboursOf(ctx, best[:16], table_dev, n, d)
                if opt.render:                                        # sample.lua:118, from the table where it lies
                    from . import render
                    with nn_utils.DeviceTensor(ctx, best[:16].shape) as bt:
                        ctx.upload(best[:16], bt.ptr)
                        render.neighbours_grid(bt, np.arange(len(idx)), nn_utils.DeviceTensor(ctx, shape, table_dev), idx[:, 0], opt.colorSpace,
                                               path=os.path.join(opt.writeTo, "best_%04d_neighbours_base.png" % run))
                # the rows found: --data has them on the host; the loader's table gives up just these
                found = data[idx[:, 0]] if table is None else np.stack([ctx.download(table_dev + 4 * d * int(j), shape[1:]) for j in idx[:, 0]])
            finally:
                if table is None:
                    ctx.free(table_dev)
            out.update(neighbour_idx=idx[:, 0], neighbour_dist=dist[:, 0], neighbours=found)
        path = os.path.join(opt.writeTo, "samples_%04d.npz" % run)
        np.savez(path, **out)
        written.append(path)
        print(f"run {run}/{opt.runs}: {path}")
    if table is not None:
        table.free()
    print("Finished.")
    return written


if __name__ == "__main__":
    main()
