"""Mirror of the reference's pretrain_g.lua: train G as the decoder half of an autoencoder (create_G_encoder -> create_G) under
nn.MSECriterion, the L1 / L2 penalty, the gradient clamp and optim.adam (pretrain_g.lua:82-206), and save the decoder as
<save>/g_pretrained_CxHxW_ndN.net - the file train.lua:148-161 (ganrev.train --G_pretrained_dir) starts G from.

    python -m ganrev.pretrain_g --epochs 2 --N_epoch 30 --batchSize 128 --save logs [--dataset DIR | --data images.npy] [--compat]

Same option names and defaults as pretrain_g.lua:12-35 for what is mirrored.  Training images come from --data (an
[N x C x H x W] float32 .npy in [0, 1]) or, without it, from synth.synthetic_images, or from --dataset DIR through ganrev.dataset (DATASET.loadRandomImages per epoch, :118).  With
--colorSpace yuv | hsl the images are rgb and are converted once per epoch load, on the device (nn_utils.rgbToColorSpace, as
dataset.lua:153 does per image); three-channel --data with --colorSpace y is converted the same way.

Two loops, as in ganrev.train_r / ganrev.train:
  fast (default)  - the epoch's images device-resident; per batch forward_dev -> gr_mse_dev -> backward_dev -> gr_adam_step
                    (penalty, clamp and Adam fused), parameters pulled to the host only before a save;
  --compat        - the fevalG closure exactly as pretrain_g.lua:148-180 spells it, over optim.adam.

--progress writes visualizeProgress (pretrain_g.lua:216-246) after every epoch from the device-resident autoencoder (ganrev.progress):
<save>/progress/real_<epoch>.png and decoded_<epoch>.png (the epoch's first 100 images and their encode-decode) and
<save>/plot_data.json (epoch, loss); the trained parameters are bit for bit those of a run without it.  Refused with --compat.

Stated deviations:
  - pretrain_g.lua:112 stops when `OPT.epochs > EPOCH`: inverted, it breaks at once for any --epochs > 1 and runs forever with
    -1.  Here --epochs N plays N epochs.
  - One more save after the last epoch, as ganrev.train does (the reference is stopped by hand).
"""
import argparse
import os
import time

import numpy as np

from . import _lib as L
from . import device, models, nn, nn_utils, optim, progress, scripts, t7
from .adversarial import penalise_and_clamp
from .synth import synthetic_images


def parse(argv=None):
    p = argparse.ArgumentParser(description="pretrain_g.lua options (pretrain_g.lua:12-35)")
    p.add_argument("--save", default="logs")                       # pretrain_g.lua:13
    p.add_argument("--saveFreq", type=int, default=30)             # :14
    p.add_argument("--epochs", type=int, default=1, help="epochs to play (see the stop-test deviation above)")
    p.add_argument("--batchSize", type=int, default=128)           # :18
    p.add_argument("--N_epoch", type=int, default=30)              # :19
    p.add_argument("--G_L1", type=float, default=0.0)              # :20
    p.add_argument("--G_L2", type=float, default=0.0)              # :21
    p.add_argument("--G_clamp", type=float, default=5.0)           # :22
    p.add_argument("--noiseDim", type=int, default=100)            # :26
    p.add_argument("--seed", type=int, default=1)                  # :29
    p.add_argument("--colorSpace", default="rgb", choices=["rgb", "y", "yuv", "hsl"])      # :30 (yuv / hsl / y from rgb images: nn_utils.rgbToColorSpace)
    p.add_argument("--height", type=int, default=32)               # :31
    p.add_argument("--width", type=int, default=32)                # :32
    p.add_argument("--data", default="", help="[N x C x H x W] float32 .npy of training images; default: synthetic")
    scripts.add_dataset_options(p)                                 # :15 --dataset
    p.add_argument("--compat", action="store_true")
    scripts.add_progress_option(p)
    p.add_argument("--conv-mode", default="f16x3", choices=["f32", "bf16x6", "f16x3"])
    p.add_argument("--quiet", action="store_true")
    return p.parse_args(argv)


def image_dims(OPT):
    return scripts.image_dims(OPT.colorSpace, OPT.height, OPT.width)         # pretrain_g.lua:49-53


def checkpoint_name(dims, noiseDim):
    """pretrain_g.lua:190 / train.lua:148: g_pretrained_CHANNELSxHEIGHTxWIDTH_ndNOISEDIM.net"""
    return "g_pretrained_%s.net" % scripts.geometry(dims, noiseDim)


def build(dims, noiseDim, seed):
    """pretrain_g.lua:82-88: G_AUTOENCODER = Sequential(G_ENCODER, G_DECODER).  No nn.Concat: it compiles as one gr_net."""
    enc = models.create_G_encoder(dims, noiseDim, True, seed)
    dec = models.create_G(dims, noiseDim, True, seed + 1)
    ae = nn.Sequential()
    ae.add(enc)
    ae.add(dec)
    ae.training()
    return ae


class DeviceLoop:
    """The fast loop: one autoencoder step per batch on device tensors (pretrain_g.lua:148-183 without a host round trip)."""

    def __init__(self, ae, dims, B, hyper):
        self.ae, self.B, self.hyper, self.t = ae, int(B), hyper, 0
        self.ctx = ae.device_net(dims).ctx             # compiled, parameters uploaded, training mode; no forward (no BatchNorm side effect)
        self.net = device.DeviceModel(self.ctx, ae)
        self.net.adam_reset()
        self.n = self.B * int(np.prod(dims))
        self.mem = device.Buffers(self.ctx)
        self.images = None
        self.grad = self.mem.malloc(4 * self.n)
        self.loss = self.mem.malloc(64)

    def load(self, images, colorSpace="rgb"):
        """the epoch's TRAIN_DATA, device-resident (pretrain_g.lua:118); rgb images are converted to colorSpace there (dataset.lua:153).
        images: a host array, uploaded, or the device table a cached dataset leaves (an owned nn_utils.DeviceTensor), which the loop takes
        over as it is; either way the previous epoch's table is freed"""
        if self.images is not None:
            self.mem.free(self.images)
        if isinstance(images, nn_utils.DeviceTensor):
            assert images.owned and images.ctx is self.ctx
            self.images, images.owned = self.mem.adopt(images.ptr, 4 * images.size), False
        else:
            images = np.ascontiguousarray(images, np.float32)
            self.images = self.ctx.upload(images, self.mem.malloc(images.nbytes))
        self.n_images = images.shape[0]
        if scripts.needs_conversion(images, colorSpace):
            n, _, h, w = images.shape
            if colorSpace == "y":             # three planes in, one out: a buffer of its own
                rgb, self.images = self.images, self.mem.malloc(4 * n * h * w)
                self.ctx.colorspace_dev(rgb, L.GR_CS_RGB, L.GR_CS_Y, n, h, w, self.images)
                self.ctx.synchronize()
                self.mem.free(rgb)
            else:                             # yuv / hsl: in place
                self.ctx.colorspace_dev(self.images, L.GR_CS_RGB, L.COLOR_SPACES[colorSpace], n, h, w, self.images)

    def batch(self, b, want_loss=False):
        x = self.images + 4 * self.n * b
        self.t += 1
        self.net.zero_grads()                                             # :151
        out = self.net.forward(x, self.B)                                 # :154
        self.ctx.mse_dev(out, x, self.n, self.loss, self.grad)            # :155,159  (targets = inputs)
        self.net.backward(self.grad, self.B, False)                       # :160 (no gradInput)
        self.net.adam_step(self.hyper, self.t)                            # :163-183 penalty, clamp, optim.adam
        return self.ctx.read_loss(self.loss) if want_loss else None

    def sync_to_host(self):
        self.ae.pull_params()                                             # parameters and BatchNorm running statistics

    def close(self):
        self.net.close()
        self.mem.close()
        self.images = None


def compat_epoch(OPT, ae, PARAMETERS, GRAD_PARAMETERS, CRITERION, OPTSTATE, TRAIN_DATA, dims):
    """pretrain_g.lua:133-185 on host tensors"""
    B = OPT.batchSize
    for batchIdx in range(1, OPT.N_epoch + 1):
        batchStart = (batchIdx - 1) * B
        inputs = np.ascontiguousarray(TRAIN_DATA[batchStart:batchStart + B], np.float32)     # :144-147
        targets = inputs.copy()

        def fevalG(x):
            if x is not PARAMETERS:
                PARAMETERS[...] = x
            GRAD_PARAMETERS[...] = 0                                      # :151
            outputs = ae.forward(inputs).copy()                           # :154
            f = CRITERION.forward(outputs, targets)                       # :155
            df_do = CRITERION.backward(outputs, targets)                  # :159
            ae.backward(inputs, df_do)                                    # :160
            f = penalise_and_clamp(PARAMETERS, GRAD_PARAMETERS, f, OPT.G_L1, OPT.G_L2, OPT.G_clamp)      # :163-175
            return f, GRAD_PARAMETERS
        optim.adam(fevalG, PARAMETERS, OPTSTATE, model=ae)                # :180
    return CRITERION.output


def save(OPT, ae, dims, epoch):
    """pretrain_g.lua:187-203: torch.save(<save>/g_pretrained_..., {G = G_AUTOENCODER:get(2), opt = OPT, EPOCH = EPOCH + 1})"""
    filename = os.path.join(OPT.save, checkpoint_name(dims, OPT.noiseDim))
    os.makedirs(OPT.save or ".", exist_ok=True)
    if not OPT.quiet:
        print("<trainer> saving network to %s" % filename)
    t7.save_checkpoint(filename, G=ae.get(2), opt=scripts.opt_table(OPT), EPOCH=epoch + 1)      # opt.colorSpace: train_r --G reads it
    return filename


def main(argv=None):
    OPT = parse(argv)
    scripts.refuse_progress_in_compat(OPT)
    dims = image_dims(OPT)
    ctx = L.default_context()
    ctx.set_conv_mode(OPT.conv_mode)
    ae = build(dims, OPT.noiseDim, OPT.seed)
    ae._ctx = ctx
    if not OPT.quiet:
        print("G autoencoder:")
        print(ae)
        print("Number of free parameters in G (total): %d" % ae._param_count())
    data = np.load(OPT.data).astype(np.float32) if OPT.data else None
    DATASET = scripts.open_dataset(OPT, "rgb", OPT.height, OPT.width, ctx)      # :60-64; rgb: the loops convert to --colorSpace as they do for --data
    nLoad = OPT.N_epoch * OPT.batchSize                                   # :117
    if OPT.compat:
        CRITERION = nn.MSECriterion()                                     # :94
        PARAMETERS, GRAD_PARAMETERS = ae.getParameters()                  # :97
        OPTSTATE = {}                                                     # :100
        loop = None
    else:
        loop = DeviceLoop(ae, dims, OPT.batchSize, L.Hyper(l1=OPT.G_L1, l2=OPT.G_L2, clamp=OPT.G_clamp))
    pictures = progress.AutoencoderPictures(loop, dims, OPT.colorSpace, OPT.save) if OPT.progress else None
    EPOCH, last, path, t0 = 1, None, None, time.perf_counter()
    try:
        for _ in range(OPT.epochs):                                       # pretrain_g.lua:112's stop test, not inverted (module docstring)
            if not OPT.quiet:
                print("<trainer> Epoch %d" % EPOCH)
            if DATASET is not None:
                TRAIN_DATA = scripts.load_random_images(DATASET, nLoad)       # :118
            elif data is not None:
                TRAIN_DATA = data[((EPOCH - 1) * nLoad + np.arange(nLoad)) % len(data)]
            else:
                TRAIN_DATA = synthetic_images(nLoad, dims, OPT.seed * 7919 + EPOCH * 3)
            if loop is None:
                if scripts.needs_conversion(TRAIN_DATA, OPT.colorSpace):
                    TRAIN_DATA = nn_utils.rgbToColorSpace(np.ascontiguousarray(TRAIN_DATA, np.float32), OPT.colorSpace)
                last = compat_epoch(OPT, ae, PARAMETERS, GRAD_PARAMETERS, CRITERION, OPTSTATE, TRAIN_DATA, dims)
            else:
                loop.load(TRAIN_DATA, OPT.colorSpace)
                for b in range(OPT.N_epoch):
                    res = loop.batch(b, want_loss=b == OPT.N_epoch - 1)
                    if res is not None:
                        last = res
            if not OPT.quiet:
                print("<trainer> last batch loss: %.4f" % last)
            if pictures is not None:
                pictures.visualize(EPOCH, last)                           # :125-127, after the epoch
            if EPOCH % OPT.saveFreq == 0:                                 # :187
                if loop is not None:
                    loop.sync_to_host()
                else:
                    ae.pull_params()
                path = save(OPT, ae, dims, EPOCH)
            EPOCH += 1
        if loop is not None:
            loop.sync_to_host()
        else:
            ae.pull_params()
        path = save(OPT, ae, dims, EPOCH - 1)                              # deviation: a final save, as ganrev.train
        if not OPT.quiet:
            print("<trainer> %.1f images/s" % (OPT.epochs * nLoad / (time.perf_counter() - t0)))
    finally:
        if pictures is not None:
            pictures.close()
        if loop is not None:
            loop.close()
    return dict(path=path, last_loss=last, model=ae, epoch=EPOCH - 1, pictures=pictures)


if __name__ == "__main__":
    main()
