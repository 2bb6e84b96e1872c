"""Train a variational autoencoder next to G and R (new: the reference has no such script; its README lists "Compare to Autoencoders, especially
VAEs" first under further research).  The encoder is models.create_VAE_encoder - create_G_encoder's trunk under a (mu | logvar) head - the decoder
is create_G, the layer between them gr_vae_sample_dev / gr_vae_sample_backward_dev (ganrev.vae), the loss

    criterion(decoder(z), x) + klWeight * mean_i KL_i,      z = mu + exp(logvar / 2) eps

under the L1 / L2 penalty, the gradient clamp and optim.adam of pretrain_g.lua:162-183.  Modelled on ganrev.pretrain_g: its option names, dataset
options, per-epoch image loading (colour-space conversion on the device), stop test and final save.

    python -m ganrev.train_vae --epochs 2 --N_epoch 30 --batchSize 128 --save logs [--dataset DIR | --data images.npy] [--criterion mse|bce] [--compat]
    python -m ganrev.apply_r --G logs/vae_3x32x32_nd100.net --R logs/vae_r_3x32x32_nd100.net --R_fixer logs/vae_r_3x32x32_nd100.net

It writes two ordinary checkpoints:
  <save>/vae_CxHxW_ndN.net     {G = the decoder, E = the whole encoder, opt, EPOCH}: a --G file for apply_r / train_r (opt carries noiseDim, height,
                               width and colorSpace)
  <save>/vae_r_CxHxW_ndN.net   {R = vae.mean_reverser(encoder), opt}: the encoder cut to its mu half, an --R file

Two loops, as in ganrev.pretrain_g:
  fast (default)  - the epoch's images device-resident; encoder and decoder run as two device.DeviceModel with the sampling layer between them.
                    Per batch: zero_grads on both; h = enc.forward(x); eps = gr_fill_normal_dev; gr_vae_sample_dev; xhat = dec.forward(z); the
                    criterion; gz = dec.backward(grad, want_gin); gr_vae_sample_backward_dev; enc.backward(gh); gr_adam_step on both.
  --compat        - the same step spelled on host tensors: forward / backward of the two nets, vae.Sample, penalise_and_clamp, optim.adam, with
                    the same eps (the device fill, downloaded).

eps of step t (1-based, counted over the whole run) is gr_fill_normal_dev with the seed eps_seed(--seed, t) = seed * 1000003 + t.

--criterion: mse (nn.MSECriterion, the default) or bce (nn.BCECriterion: G ends in a Sigmoid; the images must lie in [0, 1], which rgb and y do).
--klWeight defaults to 1 / (C H W): with the mean-reduced MSE that is, up to a constant factor, the weight of a unit-scale pixel likelihood.  It is a
knob, not a measured optimum.  --klWarmup N ramps the weight linearly from 0 over the first N batches: step t runs with
klWeight * min(1, (t - 1) / N).  The weight is a kernel argument, so the ramp costs nothing.

Out of scope: data-parallel training (kl_weight / B is the local batch's), --progress pictures (apply_r --render draws from the checkpoints), a
learned decoder variance, create_G4 as the decoder.
"""
import argparse
import os
import time

import numpy as np

from . import _lib as L
from . import device, models, nn, nn_utils, optim, pretrain_g, scripts, t7, vae
from .adversarial import penalise_and_clamp
from .synth import synthetic_images


def parse(argv=None):
    p = argparse.ArgumentParser(description="pretrain_g.lua's options (pretrain_g.lua:12-35) and the VAE's own")
    p.add_argument("--save", default="logs")
    p.add_argument("--saveFreq", type=int, default=30)
    p.add_argument("--epochs", type=int, default=1, help="epochs to play")
    p.add_argument("--batchSize", type=int, default=128)
    p.add_argument("--N_epoch", type=int, default=30)
    p.add_argument("--G_L1", type=float, default=0.0)
    p.add_argument("--G_L2", type=float, default=0.0)
    p.add_argument("--G_clamp", type=float, default=5.0)
    p.add_argument("--noiseDim", type=int, default=100)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--colorSpace", default="rgb", choices=["rgb", "y", "yuv", "hsl"])
    p.add_argument("--height", type=int, default=32)
    p.add_argument("--width", type=int, default=32)
    p.add_argument("--data", default="", help="[N x C x H x W] float32 .npy of training images; default: synthetic")
    scripts.add_dataset_options(p)
    p.add_argument("--criterion", default="mse", choices=["mse", "bce"], help="the reconstruction term: nn.MSECriterion or nn.BCECriterion")
    p.add_argument("--klWeight", type=float, default=None, help="weight of the mean KL term; default 1 / (channels * height * width)")
    p.add_argument("--klWarmup", type=int, default=0, help="ramp the KL weight linearly from 0 over the first N batches")
    p.add_argument("--compat", action="store_true")
    p.add_argument("--conv-mode", default="f16x3", choices=["f32", "bf16x6", "f16x3"])
    p.add_argument("--quiet", action="store_true")
    return p.parse_args(argv)


def image_dims(OPT):
    return scripts.image_dims(OPT.colorSpace, OPT.height, OPT.width)


def checkpoint_name(dims, noiseDim):
    """vae_CHANNELSxHEIGHTxWIDTH_ndNOISEDIM.net: the decoder as G, the encoder as E"""
    return "vae_%s.net" % scripts.geometry(dims, noiseDim)


def reverser_checkpoint_name(dims, noiseDim):
    """vae_r_CHANNELSxHEIGHTxWIDTH_ndNOISEDIM.net: the encoder's mu half as R"""
    return "vae_r_%s.net" % scripts.geometry(dims, noiseDim)


def default_kl_weight(dims):
    return 1.0 / float(int(dims[0]) * int(dims[1]) * int(dims[2]))


def kl_weight_at(weight, warmup, t):
    """the KL weight of step t (1-based): weight * min(1, (t - 1) / warmup), weight itself without a warm-up"""
    return float(weight) if warmup <= 0 else float(weight) * min(1.0, (t - 1) / float(warmup))


def eps_seed(seed, t):
    """the gr_fill_normal_dev seed of step t's eps"""
    return int(seed) * 1000003 + int(t)


def build(dims, noiseDim, seed):
    """(encoder, decoder) in training mode, seeded as pretrain_g.build seeds its two halves"""
    enc = models.create_VAE_encoder(dims, noiseDim, True, seed)
    dec = models.create_G(dims, noiseDim, True, seed + 1)
    enc.training()
    dec.training()
    return enc, dec


class DeviceLoop:
    """The fast loop: one VAE step per batch on device tensors, two DeviceModels with the sampling layer between them."""

    def __init__(self, enc, dec, dims, noiseDim, B, hyper, criterion="mse", seed=1, kl_weight=None, kl_warmup=0):
        self.enc_model, self.dec_model, self.B, self.nd, self.hyper, self.t = enc, dec, int(B), int(noiseDim), hyper, 0
        self.criterion, self.seed, self.kl_warmup = criterion, int(seed), int(kl_warmup)
        self.kl_weight = default_kl_weight(dims) if kl_weight is None else float(kl_weight)
        self.ctx = enc.device_net(dims).ctx            # compiled, parameters uploaded, training mode; no forward (no BatchNorm side effect)
        dec.device_net((self.nd,))
        self.enc, self.dec = device.DeviceModel(self.ctx, enc), device.DeviceModel(self.ctx, dec)
        self.enc.adam_reset()
        self.dec.adam_reset()
        self.n = self.B * int(np.prod(dims))
        self.mem = device.Buffers(self.ctx)
        self.images = None
        self.eps = self.mem.malloc(4 * self.B * self.nd)
        self.z = self.mem.malloc(4 * self.B * self.nd)
        self.gh = self.mem.malloc(8 * self.B * self.nd)
        self.grad = self.mem.malloc(4 * self.n)
        self.loss = self.mem.malloc(64)
        self.kl = self.mem.malloc(64)

    load = pretrain_g.DeviceLoop.load                  # the epoch's images, device-resident and in --colorSpace: the same code, not a copy of it

    def forward(self, b, eps_host=None):
        """zero_grads, encoder, eps, the sampling layer, decoder and the criterion on batch b of the loaded images; eps_host [B x noiseDim] replaces
        the drawn eps (tests)"""
        self.x = x = self.images + 4 * self.n * b
        B, nd = self.B, self.nd
        self.t += 1
        self.enc.zero_grads()
        self.dec.zero_grads()
        self.h = self.enc.forward(x, B)
        if eps_host is None:
            self.ctx.fill_normal(self.eps, B * nd, eps_seed(self.seed, self.t))
        else:
            self.ctx.upload(np.ascontiguousarray(eps_host, np.float32).reshape(B * nd), self.eps)
        self.ctx.vae_sample_dev(self.h, self.eps, B, nd, self.z, None, self.kl)
        self.out = self.dec.forward(self.z, B)
        if self.criterion == "bce":
            self.ctx.bce_dev(self.out, x, self.n, self.loss, self.grad)
        else:
            self.ctx.mse_dev(self.out, x, self.n, self.loss, self.grad)

    def backward(self):
        """decoder (with its input gradient), the sampling layer under this step's KL weight, encoder"""
        w = kl_weight_at(self.kl_weight, self.kl_warmup, self.t)
        gz = self.dec.backward(self.grad, self.B, True)
        self.ctx.vae_sample_backward_dev(self.h, self.eps, gz, self.B, self.nd, w, self.gh)
        self.enc.backward(self.gh, self.B, False)

    def step(self):
        self.enc.adam_step(self.hyper, self.t)         # penalty, clamp, optim.adam
        self.dec.adam_step(self.hyper, self.t)

    def batch(self, b, want_loss=False, eps_host=None):
        """one VAE step on batch b -> (criterion, KL mean) when asked"""
        self.forward(b, eps_host)
        self.backward()
        self.step()
        return (self.ctx.read_loss(self.loss), self.ctx.read_loss(self.kl)) if want_loss else None

    def sync_to_host(self):
        self.enc_model.pull_params()                   # parameters and BatchNorm running statistics
        self.dec_model.pull_params()

    def close(self):
        self.enc.close()
        self.dec.close()
        self.mem.close()
        self.images = None


class CompatLoop:
    """--compat: the step of DeviceLoop.batch on host tensors, the closures over optim.adam as pretrain_g.compat_epoch spells its own.  The two nets
    keep a flat parameter vector and an Adam state each: penalty, clamp and Adam are element-wise, so that is the step on their concatenation."""

    def __init__(self, OPT, enc, dec, dims, ctx):
        self.OPT, self.enc, self.dec, self.ctx, self.t = OPT, enc, dec, ctx, 0
        self.kl_weight = default_kl_weight(dims) if OPT.klWeight is None else float(OPT.klWeight)
        self.CRITERION = nn.BCECriterion() if OPT.criterion == "bce" else nn.MSECriterion()
        self.sample = vae.Sample(ctx)
        self.PE, self.GE = enc.getParameters()
        self.PD, self.GD = dec.getParameters()
        self.STATE_E, self.STATE_D = {}, {}
        self.eps_dev = ctx.malloc(4 * OPT.batchSize * OPT.noiseDim)

    def draw_eps(self, t):
        B, nd = self.OPT.batchSize, self.OPT.noiseDim
        self.ctx.fill_normal(self.eps_dev, B * nd, eps_seed(self.OPT.seed, t))
        return self.ctx.download(self.eps_dev, (B, nd))

    def batch(self, inputs, eps_host=None):
        OPT, enc, dec, sample, CRITERION = self.OPT, self.enc, self.dec, self.sample, self.CRITERION
        PE, GE, PD, GD = self.PE, self.GE, self.PD, self.GD
        self.t += 1
        w = kl_weight_at(self.kl_weight, OPT.klWarmup, self.t)
        eps = self.draw_eps(self.t) if eps_host is None else np.ascontiguousarray(eps_host, np.float32)
        targets = inputs.copy()

        def fevalE(x):                                 # the whole step: it leaves the decoder's gradient in GD
            if x is not PE:
                PE[...] = x
            GE[...] = 0
            GD[...] = 0
            h = enc.forward(inputs).copy()
            z = sample.forward(h, eps)
            outputs = dec.forward(z).copy()
            f = CRITERION.forward(outputs, targets) + w * sample.kl
            df_do = CRITERION.backward(outputs, targets)
            gz = dec.backward(z, df_do)
            gh = sample.backward(gz, w)
            enc.backward(inputs, gh)
            return penalise_and_clamp(PE, GE, f, OPT.G_L1, OPT.G_L2, OPT.G_clamp), GE

        def fevalD(x):
            if x is not PD:
                PD[...] = x
            return penalise_and_clamp(PD, GD, 0.0, OPT.G_L1, OPT.G_L2, OPT.G_clamp), GD
        optim.adam(fevalE, PE, self.STATE_E, model=enc)
        optim.adam(fevalD, PD, self.STATE_D, model=dec)
        return CRITERION.output, sample.kl

    def close(self):
        self.ctx.free(self.eps_dev)


def save(OPT, enc, dec, dims, epoch):
    """-> (the vae file, the reverser file); the host modules must be current (sync_to_host / pull_params)"""
    os.makedirs(OPT.save or ".", exist_ok=True)
    path = os.path.join(OPT.save, checkpoint_name(dims, OPT.noiseDim))
    rpath = os.path.join(OPT.save, reverser_checkpoint_name(dims, OPT.noiseDim))
    if not OPT.quiet:
        print("<trainer> saving networks to %s and %s" % (path, rpath))
    t7.save_checkpoint(path, G=dec, E=enc, opt=scripts.opt_table(OPT), EPOCH=epoch + 1)      # opt.noiseDim / height / width / colorSpace: apply_r --G reads them
    t7.save_checkpoint(rpath, R=vae.mean_reverser(enc), opt=scripts.opt_table(OPT))
    return path, rpath


def main(argv=None):
    OPT = parse(argv)
    dims = image_dims(OPT)
    if OPT.klWeight is None:
        OPT.klWeight = default_kl_weight(dims)                               # the resolved value goes into the checkpoints' opt
    if not 1 <= OPT.noiseDim <= L.Context.VAE_MAX_ND:
        raise L.GanrevError(f"--noiseDim {OPT.noiseDim}: the sampling layer takes 1 .. {L.Context.VAE_MAX_ND} dimensions")
    ctx = L.default_context()
    ctx.set_conv_mode(OPT.conv_mode)
    enc, dec = build(dims, OPT.noiseDim, OPT.seed)
    enc._ctx = dec._ctx = ctx
    if not OPT.quiet:
        print("VAE encoder:")
        print(enc)
        print("VAE decoder:")
        print(dec)
        print("Number of free parameters (encoder, decoder): %d, %d" % (enc._param_count(), dec._param_count()))
    data = np.load(OPT.data).astype(np.float32) if OPT.data else None
    DATASET = scripts.open_dataset(OPT, "rgb", OPT.height, OPT.width, ctx)      # rgb: the loops convert to --colorSpace as they do for --data
    nLoad = OPT.N_epoch * OPT.batchSize
    if OPT.compat:
        loop, compat = None, CompatLoop(OPT, enc, dec, dims, ctx)
    else:
        compat = None
        loop = DeviceLoop(enc, dec, dims, OPT.noiseDim, OPT.batchSize, L.Hyper(l1=OPT.G_L1, l2=OPT.G_L2, clamp=OPT.G_clamp), OPT.criterion, OPT.seed,
                          OPT.klWeight, OPT.klWarmup)
    EPOCH, last, paths, t0 = 1, None, None, time.perf_counter()

    def pull():
        if loop is not None:
            loop.sync_to_host()
        else:
            enc.pull_params()
            dec.pull_params()
    try:
        for _ in range(OPT.epochs):                                           # the stop test of ganrev.pretrain_g: --epochs N plays N epochs
            if not OPT.quiet:
                print("<trainer> Epoch %d" % EPOCH)
            if DATASET is not None:
                TRAIN_DATA = scripts.load_random_images(DATASET, nLoad)
            elif data is not None:
                TRAIN_DATA = data[((EPOCH - 1) * nLoad + np.arange(nLoad)) % len(data)]
            else:
                TRAIN_DATA = synthetic_images(nLoad, dims, OPT.seed * 7919 + EPOCH * 3)
            if loop is None:
                if scripts.needs_conversion(TRAIN_DATA, OPT.colorSpace):
                    TRAIN_DATA = nn_utils.rgbToColorSpace(np.ascontiguousarray(TRAIN_DATA, np.float32), OPT.colorSpace)
                for b in range(OPT.N_epoch):
                    last = compat.batch(np.ascontiguousarray(TRAIN_DATA[b * OPT.batchSize:(b + 1) * OPT.batchSize], np.float32))
            else:
                loop.load(TRAIN_DATA, OPT.colorSpace)
                for b in range(OPT.N_epoch):
                    res = loop.batch(b, want_loss=b == OPT.N_epoch - 1)
                    if res is not None:
                        last = res
            if not OPT.quiet:
                print("<trainer> last batch: criterion %.4f, KL %.4f" % last)
            if EPOCH % OPT.saveFreq == 0:
                pull()
                paths = save(OPT, enc, dec, dims, EPOCH)
            EPOCH += 1
        pull()
        paths = save(OPT, enc, dec, dims, EPOCH - 1)                           # a final save, as ganrev.pretrain_g
        if not OPT.quiet:
            print("<trainer> %.1f images/s" % (OPT.epochs * nLoad / (time.perf_counter() - t0)))
    finally:
        if loop is not None:
            loop.close()
        if compat is not None:
            compat.close()
    steps = OPT.epochs * OPT.N_epoch
    last_loss = None if last is None else last[0] + kl_weight_at(OPT.klWeight, OPT.klWarmup, steps) * last[1]
    return dict(path=paths[0], reverser_path=paths[1], last_loss=last_loss, last_criterion=None if last is None else last[0],
                last_kl=None if last is None else last[1], encoder=enc, decoder=dec, epoch=EPOCH - 1)


if __name__ == "__main__":
    main()
