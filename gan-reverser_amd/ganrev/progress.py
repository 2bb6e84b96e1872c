"""The trainers' progress pictures (`visualizeProgress` of train.lua:268-319, pretrain_with_previous_net.lua:270-306,
pretrain_g.lua:216-246 and the every-25th-batch picture of train_r.lua:207-220), drawn from the device-resident models in the middle of
a training run - and without a trace in it.

Two things make that possible.  observing() puts the compiled nets into evaluate() mode for the look and afterwards restores their mode
AND their Philox forward-call counters (gr_net_get / set_forward_counter): every forward ticks that counter and the Dropout masks of all
later batches depend on it, so without the restore a run with pictures would train differently from a run without them.  And the
pictures are rendered where the images lie: G's images, the table D ranks and the loaded training images stay on the device, the grids
are gr_progress_grid_dev = NN_UTILS.imagesToGridTensor (a fixed grid of cells, the epoch in 3 x 5-pixel digits below them), and what
comes to the host is D's predictions and the finished 8-bit grids, written as PNG (ganrev.png).  No pull_params, no host forward.

Files (START = the run's start time in seconds, as train.lua's START_TIME):
    train                         <save>/images/<START>_<epoch %05d>.png         10 x 10   G's images from VIS_NOISE_INPUTS
                                  <save>/images_good/..., <save>/images_bad/...   7 x 7    what D rates best / worst among them
                                  <save>/images_train/...                         8 x 7    the first 50 training images
    pretrain_with_previous_net    <save>/progress/images|good|bad_<batch %05d>.png         every 10th batch
    pretrain_g                    <save>/progress/real|decoded_<epoch %05d>.png            after every epoch
    train_r                       <save>/progress/pairs_<batch %05d>.png                   every 25th batch: image, G(R(image)), ...
The pictures the reference only sends to `display` (the last three scripts) are 10 cells wide and carry the batch or epoch number as
digits.  PLOT_DATA has no chart renderer here: it is written as <save>/plot_data.json = {"script", "labels", "data": rows}.
"""
import contextlib
import json
import os
import time

import numpy as np

from . import _lib as L
from . import device, nn_utils, png, synth

VIS_ROWS = 100                     # train.lua:204  NN_UTILS.createNoiseInputs(100)
PLOT_LABELS = {"train": ["epoch", "loss D", "loss G"],
               "pretrain_g": ["epoch", "G Loss"],                                                   # pretrain_g.lua:244
               "train_r": ["epoch", "R loss (low)", "R loss (avg)", "R loss (high)"]}                # train_r.lua:204


# ------------------------------------------------------------------------------------------------------------- observing
def _nets(model):
    """the compiled gr_nets of a device.DeviceModel, or the plain compiled net the train_r loop drives"""
    return list(model.nets) if isinstance(model, device.DeviceModel) else [model]


@contextlib.contextmanager
def observing(*device_models):
    """m:evaluate() ... m:training() around a look at models that are being trained (train.lua:270-271,317-318), leaving no trace: every
    part's mode and Philox forward-call counter are what they were when the block ends."""
    nets = [n for m in device_models for n in _nets(m)]
    saved = [(n, n.forward_counter(), n.training) for n in nets]
    for n in nets:
        n.set_training(False)
    try:
        yield
    finally:
        for n, counter, training in saved:
            n.set_training(training)
            n.set_forward_counter(counter)


def forward_batched(ctx, model, x_dev, rows, in_features, batch, out_dev, out_features):
    """NN_UTILS.forwardBatched (utils/nn_utils.lua:5-33) through a DeviceModel or a plain compiled net: `batch` rows per forward,
    each chunk's output copied to its rows of out_dev"""
    for lo in range(0, rows, batch):
        b = min(batch, rows - lo)
        x = x_dev + 4 * lo * in_features
        o = model.forward(x, b) if isinstance(model, device.DeviceModel) else model.forward_dev(x, b)
        ctx.copy2d(out_dev + 4 * lo * out_features, out_features, o, out_features, b, out_features)


# ------------------------------------------------------------------------------------------------------------- files
def space_of(colorSpace):
    """GR_CS_* of a script's --colorSpace (gray is ganrev.train's name for y)"""
    return L.COLOR_SPACES["y" if colorSpace == "gray" else colorSpace]


def epoch_picture_path(save, kind, start, epoch):
    """train.lua:312-314  <save>/<kind>/<START_TIME>_<epoch %05d>.png"""
    return os.path.join(save, kind, "%d_%05d.png" % (start, epoch))


def progress_path(save, kind, number):
    """<save>/progress/<kind>_<batch or epoch %05d>.png: the pictures the reference only sends to `display`"""
    return os.path.join(save, "progress", "%s_%05d.png" % (kind, number))


def plot_data_path(save):
    return os.path.join(save, "plot_data.json")


def write_plot_data(save, script, data):
    """PLOT_DATA as <save>/plot_data.json: {"script", "labels", "data"}, one row of len(labels) numbers per entry"""
    labels = PLOT_LABELS[script]
    rows = [[float(v) for v in row] for row in data]
    if any(len(r) != len(labels) for r in rows):
        raise ValueError(f"plot data of {script}: rows of {len(labels)} values ({labels})")
    os.makedirs(save or ".", exist_ok=True)
    with open(plot_data_path(save), "w") as f:
        json.dump({"script": script, "labels": labels, "data": rows}, f)
    return plot_data_path(save)


def grid(ctx, table_dev, n_rows, dims, rows, grid_h, grid_w, number, from_space, path=None):
    """NN_UTILS.saveImagesAsGrid(path, toRgb(table[rows]), grid_h, grid_w, number) (utils/nn_utils.lua:544-548) from a device table
    [n_rows x C x H x W] -> uint8 [GH x GW x Cout]; from_space: GR_CS_* or -1"""
    c, h, w = dims
    cout, gh, gw = L.progress_grid_shape(c, h, w, from_space, grid_h, grid_w)
    u8_dev = ctx.malloc(cout * gh * gw)
    try:
        ctx.progress_grid_dev(table_dev, n_rows, c, h, w, from_space, rows, grid_h, grid_w, number, u8_dev=u8_dev)
        u8 = ctx.download(u8_dev, (gh, gw, cout), np.uint8)
    finally:
        ctx.free(u8_dev)
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        png.write_png(path, u8)
    return u8


def has_nan(ctx, table_dev, n, loss_dev):
    """rndImages:ne(rndImages):sum() > 0 (train.lua:303) without bringing the images down: the mean of (x - x)^2 (gr_mse_dev of the table
    against itself) is NaN exactly when a value is NaN or infinite - G ends in a Sigmoid, which has no infinity to give"""
    ctx.mse_dev(table_dev, table_dev, n, loss_dev)
    return bool(np.isnan(ctx.read_loss(loss_dev)))


def rank(ctx, d_model, table_dev, rows, npix, batch, preds_dev, nbMaxOut=50):
    """NN_UTILS.sortImagesByPrediction twice (train.lua:300-301): D over the table, `batch` rows per forward, then the orders
    -> (predictions [rows], descending order, ascending order), each order min(nbMaxOut, rows) long (nn_utils.predictionOrder)"""
    forward_batched(ctx, d_model, table_dev, rows, npix, batch, preds_dev, 1)
    preds = ctx.download(preds_dev, (rows,), np.float32)
    return preds, nn_utils.predictionOrder(preds, False, nbMaxOut), nn_utils.predictionOrder(preds, True, nbMaxOut)


# ------------------------------------------------------------------------------------------------------------- train.lua:268-319
def sanity_seed(seed, epoch):
    return seed * 7919 + epoch * 3 + 2           # beside synthetic_images' seed * 7919 + epoch * 3: another stream


def sanity_image(dims, seed, epoch):
    """train.lua:275-285: uniform(0, 0.5) noise; in channel 0 a diagonal of 1.0 and 0.5 at every fourth row / column crossing"""
    img = synth.uniform(dims, sanity_seed(seed, epoch), 0.0, 0.5)
    i, j = np.mgrid[0:dims[1], 0:dims[2]]
    img[0][((i + 1) % 4 == 0) & ((j + 1) % 4 == 0)] = 0.5
    img[0][i == j] = 1.0
    return img


def vis_noise_seed(seed):
    return seed * 100003 - 1                     # the batches' noise uses seed * 100003 + 1, 2, ...


class TrainPictures:
    """visualizeProgress of train.lua:268-319 for an adversarial.DeviceGame.  VIS_NOISE_INPUTS is drawn once (or taken from a
    checkpoint: train.lua:116,204) and kept on the device; .vis_noise_inputs is its host copy for the checkpoint."""

    def __init__(self, game, dims, colorSpace, save, start=None, vis_noise_inputs=None, plot_data=None):
        self.game, self.ctx, self.dims, self.save = game, game.ctx, tuple(dims), save
        self.OPT = OPT = game.env.OPT
        self.from_space = space_of(colorSpace)
        self.start = int(time.time()) if start is None else int(start)
        self.npix = int(np.prod(self.dims))
        self.mem = device.Buffers(self.ctx)
        m = self.mem.malloc
        self.noise = m(4 * VIS_ROWS * OPT.noiseDim)
        if vis_noise_inputs is None:
            self.ctx.fill_noise(self.noise, VIS_ROWS * OPT.noiseDim, OPT.noiseMethod, vis_noise_seed(OPT.seed))
            self.vis_noise_inputs = self.ctx.download(self.noise, (VIS_ROWS, OPT.noiseDim))
        else:
            self.vis_noise_inputs = np.ascontiguousarray(vis_noise_inputs, np.float32).reshape(VIS_ROWS, OPT.noiseDim)
            self.ctx.upload(self.vis_noise_inputs, self.noise)
        self.images, self.ranked, self.train = m(4 * VIS_ROWS * self.npix), m(4 * VIS_ROWS * self.npix), m(4 * 50 * self.npix)
        self.preds, self.loss = m(4 * VIS_ROWS), m(16)
        self.plot_data = [list(r) for r in plot_data] if plot_data else []
        self.last = None                                     # what the last call saw: predictions, orders, grids, paths

    def visualize(self, TRAIN_DATA, epoch):
        """the four pictures of epoch `epoch` from the models as they stand; TRAIN_DATA: the epoch's images (train.lua:216), a host array
        or the device table a cached dataset leaves (nn_utils.DeviceTensor)"""
        ctx, OPT, npix, B = self.ctx, self.OPT, self.npix, self.OPT.batchSize
        if isinstance(TRAIN_DATA, nn_utils.DeviceTensor):
            n_train = min(50, TRAIN_DATA.shape[0])
            ctx.copy2d(self.train, npix, TRAIN_DATA.ptr, npix, n_train, npix)
        else:
            n_train = min(50, len(TRAIN_DATA))                                      # train.lua:288 (which indexes past a shorter load)
            ctx.upload(np.ascontiguousarray(TRAIN_DATA[:n_train], np.float32), self.train)
        ctx.upload(sanity_image(self.dims, OPT.seed, epoch), self.ranked + 4 * npix * (VIS_ROWS - 1))      # :299, in place in the copy
        with observing(self.game.gg, self.game.dg):                                 # :270-271 ... :317-318
            forward_batched(ctx, self.game.gg, self.noise, VIS_ROWS, OPT.noiseDim, B, self.images, npix)       # :291
            ctx.copy2d(self.ranked, npix, self.images, npix, VIS_ROWS - 2, npix)    # :297 rndImages:clone(), the rows the next lines keep
            ctx.copy2d(self.ranked + 4 * npix * (VIS_ROWS - 2), npix, self.train, npix, 1, npix)           # :298 one real face
            preds, good, bad = rank(ctx, self.game.dg, self.ranked, VIS_ROWS, npix, B, self.preds)         # :300-301
        if has_nan(ctx, self.images, VIS_ROWS * npix, self.loss):                   # :303-305
            print("[visualizeProgress] Generated images contain NaNs")
        out = dict(predictions=preds, good=good, bad=bad, paths={}, u8={})
        for kind, table, n, rows, gh, gw in (("images", self.images, VIS_ROWS, np.arange(VIS_ROWS), 10, 10),      # :312
                                             ("images_good", self.ranked, VIS_ROWS, good, 7, 7),                  # :313
                                             ("images_bad", self.ranked, VIS_ROWS, bad, 7, 7),                    # :314
                                             ("images_train", self.train, 50, np.arange(n_train), 8, 7)):         # :310
            out["paths"][kind] = epoch_picture_path(self.save, kind, self.start, epoch)
            out["u8"][kind] = grid(ctx, table, n, self.dims, rows, gh, gw, epoch, self.from_space, out["paths"][kind])
        self.last = out
        return out

    def log(self, epoch, loss_d, loss_g):
        self.plot_data.append([epoch, loss_d, loss_g])
        return write_plot_data(self.save, "train", self.plot_data)

    def close(self):
        self.mem.close()


# ------------------------------------------------------------------------------------------- pretrain_with_previous_net.lua:270-306
class DistillPictures:
    """visualizeProgress(batchIdx) for a pretrain_with_previous_net.DeviceDistill: 100 fresh images of the new G; 50 real images and
    G's first 50, ranked by the new D.  real_rgb(n) -> [n x 3 x H x W] host rgb images (converted to --colorSpace on the device)."""

    def __init__(self, loop, save):
        self.loop, self.ctx, self.save = loop, loop.ctx, save
        self.OPT = OPT = loop.s.OPT
        self.dims, self.npix = loop.dims, loop.npix
        self.mem = device.Buffers(self.ctx)
        m = self.mem.malloc
        self.noise, self.images, self.both = m(4 * VIS_ROWS * OPT.noiseDim), m(4 * VIS_ROWS * self.npix), m(4 * VIS_ROWS * self.npix)
        self.rgb, self.preds = m(4 * 50 * 3 * self.dims[1] * self.dims[2]), m(4 * VIS_ROWS)
        self.last = None

    def visualize(self, real_rgb, batchIdx):
        ctx, OPT, npix, B = self.ctx, self.OPT, self.npix, self.OPT.batchSize
        _, H, W = self.dims
        real = np.ascontiguousarray(real_rgb, np.float32)
        n_real = min(50, len(real))
        ctx.fill_noise(self.noise, VIS_ROWS * OPT.noiseDim, OPT.noiseMethod, vis_noise_seed(OPT.seed) - batchIdx)      # :275 fresh noise per call
        ctx.upload(real[:n_real], self.rgb)
        ctx.colorspace_dev(self.rgb, L.GR_CS_RGB, self.loop.cs, n_real, H, W, self.both)                  # :279-283 (dataset.lua:153)
        with observing(self.loop.gg, self.loop.dg):                                                         # :272-273 ... :304-305
            forward_batched(ctx, self.loop.gg, self.noise, VIS_ROWS, OPT.noiseDim, B, self.images, npix)   # :277
            ctx.copy2d(self.both + 4 * npix * n_real, npix, self.images, npix, VIS_ROWS - n_real, npix)    # :284-287
            preds, good, bad = rank(ctx, self.loop.dg, self.both, VIS_ROWS, npix, B, self.preds)           # :289-290
        out = dict(predictions=preds, good=good, bad=bad, paths={}, u8={})
        for kind, table, rows in (("images", self.images, np.arange(VIS_ROWS)), ("good", self.both, good), ("bad", self.both, bad)):      # :299-301
            out["paths"][kind] = progress_path(self.save, kind, batchIdx)
            out["u8"][kind] = grid(ctx, table, VIS_ROWS, self.dims, rows, -(-len(rows) // 10), 10, batchIdx, self.loop.cs, out["paths"][kind])
        self.last = out
        return out

    def close(self):
        self.mem.close()


# ------------------------------------------------------------------------------------------------------ pretrain_g.lua:216-246
class AutoencoderPictures:
    """visualizeProgress() for a pretrain_g.DeviceLoop: 100 loaded images and their encode-decode; PLOT_DATA gets {EPOCH, loss}."""

    def __init__(self, loop, dims, colorSpace, save):
        self.loop, self.ctx, self.dims, self.save = loop, loop.ctx, tuple(dims), save
        self.from_space, self.npix = space_of(colorSpace), int(np.prod(dims))
        self.mem = device.Buffers(self.ctx)
        self.decoded = self.mem.malloc(4 * VIS_ROWS * self.npix)
        self.plot_data, self.last = [], None

    def visualize(self, epoch, loss):
        """after epoch `epoch`: the first 100 of the epoch's device-resident images (pretrain_g.lua:225 loads 100 more; here potential
        training images are the ones at hand) through the autoencoder, loop.B rows per forward"""
        ctx, loop, npix = self.ctx, self.loop, self.npix
        n = min(VIS_ROWS, loop.n_images)
        with observing(loop.net):                                                                           # :218 ... :247
            forward_batched(ctx, loop.net, loop.images, n, npix, loop.B, self.decoded, npix)               # :236
        self.plot_data.append([epoch, loss])                                                                # :239
        out = dict(paths={}, u8={}, plot=write_plot_data(self.save, "pretrain_g", self.plot_data))
        for kind, table in (("real", loop.images), ("decoded", self.decoded)):                              # :242-243
            out["paths"][kind] = progress_path(self.save, kind, epoch)
            out["u8"][kind] = grid(ctx, table, n, self.dims, np.arange(n), -(-n // 10), 10, epoch, self.from_space, out["paths"][kind])
        self.last = out
        return out

    def close(self):
        self.mem.close()


# ------------------------------------------------------------------------------------------------------ train_r.lua:189-222
def loss_window_row(batchIdx, losses, every=100):
    """train_r.lua:193-203: {batchIdx, low, avg, high} of the last `every` losses"""
    window = [float(v) for v in losses[-every:]]
    return [batchIdx, min(window), sum(window) / every, max(window)]


class ReverserPictures:
    """The every-25th-batch picture of train_r.lua:207-220 and PLOT_DATA of :191-204 for the device-resident train_r loop: gnet / rnet
    are the compiled nets parallel.DeviceTrainer drives, noise_dev the batch's noise."""
    PICTURE_EVERY, PLOT_EVERY = 25, 100

    def __init__(self, ctx, gnet, rnet, dims, noiseDim, batchSize, colorSpace, save):
        self.ctx, self.gnet, self.rnet, self.dims, self.save = ctx, gnet, rnet, tuple(dims), save
        self.nd, self.B, self.from_space, self.npix = int(noiseDim), int(batchSize), space_of(colorSpace), int(np.prod(dims))
        self.mem = device.Buffers(ctx)
        self.pairs = self.mem.malloc(4 * 2 * self.B * self.npix)
        self.losses, self.plot_data, self.last = [], [], None
        write_plot_data(self.save, "train_r", self.plot_data)              # the file exists from the start; rows come every 100 batches

    def after_batch(self, batchIdx, loss, noise_dev):
        self.losses.append(loss)                                                                            # :191
        out = None
        if batchIdx % self.PLOT_EVERY == 0:                                                                 # :193-205
            self.plot_data.append(loss_window_row(batchIdx, self.losses, self.PLOT_EVERY))
            write_plot_data(self.save, "train_r", self.plot_data)
        if batchIdx % self.PICTURE_EVERY == 0:                                                              # :207-218
            ctx, npix, B = self.ctx, self.npix, self.B
            with observing(self.gnet, self.rnet):                                                           # :189 ... :222 (G is in evaluate() already)
                images = self.gnet.forward_dev(noise_dev, B)                                                # the batch's images (:139)
                ctx.copy2d(self.pairs, 2 * npix, images, npix, B, npix)                                     # :213 rows 0, 2, 4, ...
                after_r = self.rnet.forward_dev(images, B)                                                  # :208
                back = self.gnet.forward_dev(after_r, B)                                                    # :209
                ctx.copy2d(self.pairs + 4 * npix, 2 * npix, back, npix, B, npix)                            # :214 rows 1, 3, 5, ...
            path = progress_path(self.save, "pairs", batchIdx)
            u8 = grid(ctx, self.pairs, 2 * B, self.dims, np.arange(2 * B), -(-2 * B // 10), 10, batchIdx, self.from_space, path)      # :217
            out = self.last = dict(paths={"pairs": path}, u8={"pairs": u8})
        return out

    def close(self):
        self.mem.close()
