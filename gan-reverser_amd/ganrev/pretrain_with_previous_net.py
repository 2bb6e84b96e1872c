"""Mirror of the reference's pretrain_with_previous_net.lua:92-266: carry a trained G / D pair over to a new noise dimension or a
new colour space.  A fresh create_G learns to paint what the old G paints from the same noise (nn.MSECriterion on the images, the old
ones converted with NN_UTILS.switchColorSpace), a fresh create_D learns to rate what the old D rates (nn.BCECriterion against the old
D's predictions as SOFT targets), each under its L1 / L2 penalty, gradient clamp and optim.adam, and the pair is saved as
<save>/pretrained_CxHxW_ndN.net = {G, D, opt}.

    python -m ganrev.pretrain_with_previous_net --network logs/adversarial.net --N_batches 1000 --colorSpace yuv --noiseDim 64 \\
        --save logs [--dataset DIR | --data images.npy] [--compat]

Same option names and defaults as pretrain_with_previous_net.lua:12-37.  --noplot, --window, --aws, --threads and --N_epoch are
accepted and unused (the reference's `display` UI, thread count and an option its loop never reads).  Real images come from --data
(an rgb [N x 3 x H x W] float32 .npy in [0, 1], converted to --colorSpace with rgbToColorSpace as dataset.lua:153 does) or, without
it, from synth.synthetic_images, or from --dataset DIR through ganrev.dataset (DATASET.loadRandomImages(batchSize / 2) per batch, :171).
--progress writes visualizeProgress (:270-306) every 10th batch (:245-247) from the device-resident new G and D (ganrev.progress):
<save>/progress/images_<batch>.png, good_<batch>.png and bad_<batch>.png; its 50 real images are drawn beside the training stream
(a --dataset draw with a seed of its own), so the trained parameters are bit for bit those of a run without it.  Refused with --compat.

Two loops, as in ganrev.pretrain_g:
  fast (default)  - device-resident: gr_fill_*_dev for both noise tensors, gr_copy2d_dev for the shared noise columns and the two
                    halves of D's input, gr_colorspace_dev for the two conversions, the four nets through
                    device.DeviceModel, gr_mse_dev / gr_bce_dev, gr_adam_step (penalty, clamp and Adam fused).  Only the real
                    half-batch goes up and, on request, two losses come down.
  --compat        - fevalG / fevalD exactly as :185-239 spells them, on host arrays over optim.adam.

Stated deviations:
  - The noise is drawn per batch, not as one [batchSize * N_batches x noiseDim] tensor up front (:151-159): batch i uses the seeds
    (seed * 100003 + 2 i - 1, + 2 i) for the old and the new noise; the first min(noiseDim, prevNoiseDim) columns are shared as there.
  - --batchSize must be even (:171 loads batchSize / 2 real images and :177 copies batchSize / 2 generated ones: an odd size leaves
    the last row of D's input uninitialised) and the previous net's height / width must equal --height / --width (:178 copies the
    old G's images into a tensor of the new size): both are refused here, the reference silently breaks.
  - ganrev.train writes opt.colorSpace = "gray" for one channel; it is read as "y" (a reference checkpoint says "y").
"""
import argparse
import os
import time

import numpy as np

from . import _lib as L
from . import device, models, nn, nn_utils, optim, progress, scripts, t7
from .adversarial import penalise_and_clamp
from .synth import synthetic_images

COLOR_SPACES = ("rgb", "yuv", "hsl", "y")


def parse(argv=None):
    p = argparse.ArgumentParser(description="pretrain_with_previous_net.lua options (:12-37)")
    p.add_argument("--save", default="logs")                       # :13
    p.add_argument("--batchSize", type=int, default=32)            # :14
    p.add_argument("--noplot", action="store_true")                # :15 (unused: no display UI)
    p.add_argument("--window", type=int, default=23)               # :16 (unused)
    p.add_argument("--seed", type=int, default=1)                  # :17
    p.add_argument("--aws", action="store_true")                   # :18 (unused)
    p.add_argument("--saveFreq", type=int, default=50)             # :19
    p.add_argument("--gpu", type=int, default=0)                   # :20
    p.add_argument("--threads", type=int, default=8)               # :21 (unused)
    p.add_argument("--colorSpace", default="rgb", choices=COLOR_SPACES)     # :22
    p.add_argument("--height", type=int, default=32)               # :23
    p.add_argument("--width", type=int, default=32)                # :24
    p.add_argument("--G_clamp", type=float, default=5.0)           # :25
    p.add_argument("--D_clamp", type=float, default=1.0)           # :26
    p.add_argument("--G_L1", type=float, default=0.0)              # :27
    p.add_argument("--G_L2", type=float, default=0.0)              # :28
    p.add_argument("--D_L1", type=float, default=0.0)              # :29
    p.add_argument("--D_L2", type=float, default=1e-4)             # :30
    p.add_argument("--N_epoch", type=int, default=10000)           # :31 (the loop never reads it)
    p.add_argument("--noiseDim", type=int, default=100)            # :32
    p.add_argument("--noiseMethod", default="normal", choices=["normal", "uniform"])      # :33
    p.add_argument("--network", default="logs/adversarial.net")    # :34
    p.add_argument("--N_batches", type=int, default=1000)          # :35
    p.add_argument("--data", default="", help="rgb [N x 3 x H x W] float32 .npy of real images in [0, 1]; default: synthetic")      # :36 --dataset
    scripts.add_dataset_options(p)                                 # :36 --dataset
    p.add_argument("--compat", action="store_true")
    scripts.add_progress_option(p)
    p.add_argument("--conv-mode", default="f16x3", choices=["f32", "bf16x6", "f16x3"])
    p.add_argument("--quiet", action="store_true")
    return p.parse_args(argv)


image_dims = scripts.image_dims                                              # :59-63


def checkpoint_name(dims, noiseDim):
    """:262  pretrained_CHANNELSxHEIGHTxWIDTH_ndNOISEDIM.net"""
    return "pretrained_%s.net" % scripts.geometry(dims, noiseDim)


def previous_options(opt):
    """(noiseDim, noiseMethod, colorSpace, height, width) of the checkpoint's opt table (:101-105)"""
    cs = opt.get("colorSpace", "rgb")
    cs = "y" if cs == "gray" else cs                                         # ganrev.train's name for one channel
    if cs not in COLOR_SPACES:
        raise L.GanrevError(f"the previous network's opt.colorSpace '{cs}' is none of {COLOR_SPACES}")
    return int(opt["noiseDim"]), opt.get("noiseMethod", "normal"), cs, int(opt["height"]), int(opt["width"])


def check_options(OPT, prev):
    if OPT.batchSize < 2 or OPT.batchSize % 2:
        raise L.GanrevError(f"--batchSize {OPT.batchSize}: must be even (half real, half generated images: "
                            "pretrain_with_previous_net.lua:171,177)")
    if (prev[3], prev[4]) != (OPT.height, OPT.width):
        raise L.GanrevError(f"the previous network paints {prev[3]} x {prev[4]} images, --height / --width ask for {OPT.height} x {OPT.width}: "
                            "the images are copied, not scaled (pretrain_with_previous_net.lua:178)")


def noise_seeds(seed, i):
    """seeds of batch i's (1-based) old and new noise tensors"""
    return seed * 100003 + 2 * i - 1, seed * 100003 + 2 * i


def real_images(OPT, data, i, half, DATASET=None):
    """DATASET.loadRandomImages(batchSize / 2) of batch i (:171), as rgb [half x 3 x H x W]: the loader's draw from --dataset,
    consecutive images of --data, or synthetic"""
    if DATASET is not None:
        return scripts.load_random_images(DATASET, half)
    if data is not None:
        return np.ascontiguousarray(data[((i - 1) * half + np.arange(half)) % len(data)], np.float32)
    return synthetic_images(half, (3, OPT.height, OPT.width), OPT.seed * 7919 + i * 3)


def picture_images(OPT, data, i, DATASET=None):
    """imagesReal = DATASET.loadRandomImages(50) of visualizeProgress(i) (:279), as rgb [50 x 3 x H x W], WITHOUT touching what the
    batches read: a draw of the loader with a seed of its own (its draw count stays), --data from its end, or synthetic images of another seed"""
    if DATASET is not None:
        return DATASET.loadRandomImages(50, seed=[OPT.seed, 0x70726F67, i], device=False).images
    if data is not None:
        return np.ascontiguousarray(data[(len(data) - 1 - (i * 50 + np.arange(50))) % len(data)], np.float32)
    return synthetic_images(50, (3, OPT.height, OPT.width), OPT.seed * 7919 + i * 3 + 1)


def compile_models(state):
    """Compile the four networks with one forward of two samples each, WITHOUT side effects on them (device.compile_models, as
    adversarial.DeviceGame does).  Both loops start here, so their Philox dropout streams have seen the same number of forwards."""
    s = state
    s.G_PREV.evaluate(); s.D_PREV.evaluate()                                 # :98-99
    s.G.training(); s.D.training()
    device.compile_models(np.zeros((2, s.prev[0]), np.float32), s.G_PREV, s.D_PREV)
    device.compile_models(np.zeros((2, s.OPT.noiseDim), np.float32), s.G, s.D)


class DeviceDistill:
    """The fast loop: one batch of pretrain_with_previous_net.lua:161-242 on device tensors."""

    def __init__(self, state):
        s = self.s = state
        OPT = s.OPT
        self.ctx = ctx = s.G._context()
        self.B, self.half = OPT.batchSize, OPT.batchSize // 2
        self.dims, self.pdims = s.dims, image_dims(s.prev[2], s.prev[3], s.prev[4])
        self.npix, self.pnpix = int(np.prod(self.dims)), int(np.prod(self.pdims))
        self.cs, self.pcs = L.COLOR_SPACES[OPT.colorSpace], L.COLOR_SPACES[s.prev[2]]
        self.gg_prev, self.gg, self.dg_prev, self.dg = (device.DeviceModel(ctx, m) for m in (s.G_PREV, s.G, s.D_PREV, s.D))
        self.gprev, self.gnet = s.G_PREV._net, s.G._net       # the two G nets by name: not used by the loop, read by its tests
        for m in (self.gg_prev, self.dg_prev):
            m.set_training(False)
        for m in (self.gg, self.dg):
            m.set_training(True)
            m.adam_reset()
        self.mem = device.Buffers(ctx)
        B, m = self.B, self.mem.malloc
        self.prev_noise, self.noise = m(4 * B * s.prev[0]), m(4 * B * OPT.noiseDim)
        self.images_by_gprev, self.d_input, self.d_input_prev = m(4 * B * self.npix), m(4 * B * self.npix), m(4 * B * self.pnpix)
        self.real_rgb = m(4 * self.half * 3 * self.dims[1] * self.dims[2])
        self.grad_g, self.df, self.loss_g, self.loss_d = m(4 * B * self.npix), m(4 * B), m(16), m(16)
        self.hyper_g = L.Hyper(l1=OPT.G_L1, l2=OPT.G_L2, clamp=OPT.G_clamp)
        self.hyper_d = L.Hyper(l1=OPT.D_L1, l2=OPT.D_L2, clamp=OPT.D_clamp)
        self.t = 0

    def forward(self, real_rgb, prev_noise=None, noise=None):
        """:151-183: both noise tensors, the four forwards and the two conversions.  real_rgb: [batchSize / 2 x 3 x H x W] host array
        (the one upload), or a nn_utils.DeviceTensor of that shape (a draw from the dataset cache), copied on the device.
        prev_noise / noise: host noise instead of device-drawn noise (parity tests); the shared columns are copied either way."""
        s, ctx, B, half = self.s, self.ctx, self.B, self.half
        OPT, (pnd, pmethod) = s.OPT, s.prev[:2]
        _, H, W = self.dims
        self.t += 1
        device.range_guard(ctx, self.t, (self.gg_prev, self.gg, self.dg_prev, self.dg))
        s1, s2 = noise_seeds(OPT.seed, self.t)
        ctx.fill_noise(self.prev_noise, B * pnd, pmethod, s1, prev_noise)                           # :151
        ctx.fill_noise(self.noise, B * OPT.noiseDim, OPT.noiseMethod, s2, noise)                    # :152
        shared = min(OPT.noiseDim, pnd)
        ctx.copy2d(self.noise, OPT.noiseDim, self.prev_noise, pnd, B, shared)                       # :155-159
        old = self.gg_prev.forward(self.prev_noise, B)                                              # :166
        ctx.colorspace_dev(old, self.pcs, self.cs, B, H, W, self.images_by_gprev)                   # :167 (rgb -> rgb: the :clone())
        self.gg.zero_grads()
        self.images_by_g = self.gg.forward(self.noise, B)                                           # :168
        if isinstance(real_rgb, nn_utils.DeviceTensor):
            if real_rgb.size != half * 3 * H * W:
                raise L.GanrevError(f"DeviceDistill.forward: device images {real_rgb.shape} are not [{half} x 3 x {H} x {W}]")
            ctx.copy2d(self.real_rgb, 3 * H * W, real_rgb.ptr, 3 * H * W, half, 3 * H * W)
        else:
            ctx.upload(np.ascontiguousarray(real_rgb, np.float32).reshape(half, 3 * H * W), self.real_rgb)
        ctx.colorspace_dev(self.real_rgb, L.GR_CS_RGB, self.cs, half, H, W, self.d_input)           # dataset.lua:153; :173-176
        ctx.copy2d(self.d_input + 4 * half * self.npix, self.npix, self.images_by_gprev, self.npix, half, self.npix)      # :177-180
        ctx.colorspace_dev(self.d_input, self.cs, self.pcs, B, H, W, self.d_input_prev)             # :182
        self.preds_by_dprev = self.dg_prev.forward(self.d_input_prev, B)
        self.dg.zero_grads()
        self.preds_by_d = self.dg.forward(self.d_input, B)                                          # :183

    def backward(self):
        """the criterion and backward halves of fevalG (:190-194) and fevalD (:218-222)"""
        ctx, B = self.ctx, self.B
        ctx.mse_dev(self.images_by_g, self.images_by_gprev, B * self.npix, self.loss_g, self.grad_g)
        self.gg.backward(self.grad_g, B, False)
        ctx.bce_dev(self.preds_by_d, self.preds_by_dprev, B, self.loss_d, self.df)
        self.dg.backward(self.df, B, False)

    def step(self):
        """penalty, clamp (:196-208, :224-236) and optim.adam (:241-242), fused"""
        self.gg.adam_step(self.hyper_g, self.t)
        self.dg.adam_step(self.hyper_d, self.t)

    def batch(self, real_rgb, prev_noise=None, noise=None, want_loss=False):
        self.forward(real_rgb, prev_noise, noise)
        self.backward()
        self.step()
        if not want_loss:
            return None
        return self.ctx.read_loss(self.loss_g), self.ctx.read_loss(self.loss_d)

    def sync_to_host(self):
        self.s.G.pull_params()
        self.s.D.pull_params()

    def close(self):
        for m in (self.gg_prev, self.gg, self.dg_prev, self.dg, self.mem):
            m.close()


def compat_batch(state, i, real_rgb, prev_noise=None, noise=None):
    """:161-242 on host arrays, closure by closure.  Returns (loss G, loss D) = (CRITERION_G.output, CRITERION_D.output)."""
    s = state
    OPT, (pnd, pmethod, pcs) = s.OPT, s.prev[:3]
    B, half = OPT.batchSize, OPT.batchSize // 2
    ctx = s.G._context()
    s1, s2 = noise_seeds(OPT.seed, i)
    draw = lambda dim, method, seed: nn_utils.createNoiseInputsDev(ctx, B, dim, method, seed)       # the fast loop's stream, read back
    if prev_noise is None:
        t = draw(pnd, pmethod, s1); prev_noise = t.numpy(); t.free()
    if noise is None:
        t = draw(OPT.noiseDim, OPT.noiseMethod, s2); noise = t.numpy(); t.free()
    prevBatchNoise = np.ascontiguousarray(prev_noise, np.float32).reshape(B, pnd)
    batchNoise = np.array(noise, np.float32).reshape(B, OPT.noiseDim)
    shared = min(OPT.noiseDim, pnd)
    batchNoise[:, :shared] = prevBatchNoise[:, :shared]                                             # :155-159
    imagesByGprev = s.G_PREV.forward(prevBatchNoise).copy()                                         # :166
    imagesByGprev = np.array(nn_utils.switchColorSpace(imagesByGprev, pcs, OPT.colorSpace), copy=True)      # :167
    imagesByG = s.G.forward(batchNoise).copy()                                                      # :168
    imagesDinput = np.empty((B,) + s.dims, np.float32)                                              # :170
    imagesDinput[:half] = nn_utils.rgbToColorSpace(np.ascontiguousarray(real_rgb, np.float32), OPT.colorSpace)      # :171-176
    imagesDinput[half:] = imagesByGprev[:half]                                                      # :177-180
    predsByDprev = s.D_PREV.forward(nn_utils.switchColorSpace(imagesDinput, OPT.colorSpace, pcs)).copy()      # :182
    predsByD = s.D.forward(imagesDinput).copy()                                                     # :183

    def fevalG(x):
        if x is not s.PARAMETERS_G:
            s.PARAMETERS_G[...] = x
        s.GRAD_PARAMETERS_G[...] = 0                                                                # :187
        f = s.CRITERION_G.forward(imagesByG, imagesByGprev)                                         # :190
        df_do = s.CRITERION_G.backward(imagesByG, imagesByGprev)                                    # :193
        s.G.backward(batchNoise, df_do)                                                             # :194
        return penalise_and_clamp(s.PARAMETERS_G, s.GRAD_PARAMETERS_G, f, OPT.G_L1, OPT.G_L2, OPT.G_clamp), s.GRAD_PARAMETERS_G      # :196-208

    def fevalD(x):
        if x is not s.PARAMETERS_D:
            s.PARAMETERS_D[...] = x
        s.GRAD_PARAMETERS_D[...] = 0                                                                # :215
        f = s.CRITERION_D.forward(predsByD, predsByDprev)                                           # :218
        df_do = s.CRITERION_D.backward(predsByD, predsByDprev)                                      # :221
        s.D.backward(imagesDinput, df_do)                                                           # :222
        return penalise_and_clamp(s.PARAMETERS_D, s.GRAD_PARAMETERS_D, f, OPT.D_L1, OPT.D_L2, OPT.D_clamp), s.GRAD_PARAMETERS_D      # :224-236

    optim.adam(fevalG, s.PARAMETERS_G, s.OPTSTATE["adam"]["G"], model=s.G)                          # :241
    optim.adam(fevalD, s.PARAMETERS_D, s.OPTSTATE["adam"]["D"], model=s.D)                          # :242
    return s.CRITERION_G.output, s.CRITERION_D.output


class State:
    """the globals of pretrain_with_previous_net.lua:92-141"""


def setup(OPT, G_PREV, D_PREV, prev, G=None, D=None):
    """:93-141 from an already loaded previous pair; prev = previous_options(opt).  G / D: the new pair (default: create_G / create_D)."""
    check_options(OPT, prev)
    s = State()
    s.OPT, s.prev, s.G_PREV, s.D_PREV = OPT, prev, G_PREV, D_PREV
    s.dims = image_dims(OPT.colorSpace, OPT.height, OPT.width)
    s.D = D if D is not None else models.create_D(s.dims, True, OPT.seed)                           # :114
    s.G = G if G is not None else models.create_G(s.dims, OPT.noiseDim, True, OPT.seed + 1)         # :115
    ctx = L.default_context()
    for m in (s.G, s.D, s.G_PREV, s.D_PREV):
        m._ctx = ctx
    compile_models(s)
    if OPT.compat:
        s.CRITERION_G, s.CRITERION_D = nn.MSECriterion(), nn.BCECriterion()                         # :133-134
        s.PARAMETERS_G, s.GRAD_PARAMETERS_G = s.G.getParameters()                                   # :137-138
        s.PARAMETERS_D, s.GRAD_PARAMETERS_D = s.D.getParameters()
        s.OPTSTATE = {"adam": {"G": {}, "D": {}}}                                                   # :141
    return s


def save(OPT, s):
    """:260-266  torch.save(<save>/pretrained_..., {G = G, D = D, opt = OPT})"""
    filename = os.path.join(OPT.save, checkpoint_name(s.dims, OPT.noiseDim))
    os.makedirs(OPT.save or ".", exist_ok=True)
    if not OPT.quiet:
        print("Saving networks...")
    t7.save_checkpoint(filename, G=s.G, D=s.D, opt=scripts.opt_table(OPT))
    return filename


def main(argv=None):
    OPT = parse(argv)
    scripts.refuse_progress_in_compat(OPT)
    ctx = L.default_context()
    ctx.set_conv_mode(OPT.conv_mode)
    if not OPT.quiet:
        print("<trainer> reloading previously trained network: %s" % OPT.network)
    ck = scripts.load_checkpoint(OPT.network)                                                       # :95
    prev = previous_options(ck["opt"])
    s = setup(OPT, ck["G"], ck["D"], prev)
    if not OPT.quiet:
        for name, m in (("G_PREV", s.G_PREV), ("G", s.G), ("D_PREV", s.D_PREV), ("D", s.D)):
            print("Number of free parameters in %s: %d" % (name, m._param_count()))
    data = np.load(OPT.data).astype(np.float32) if OPT.data else None
    if data is not None and tuple(data.shape[1:]) != (3, OPT.height, OPT.width):
        raise L.GanrevError(f"--data holds {tuple(data.shape[1:])} images, not rgb (3, {OPT.height}, {OPT.width})")
    DATASET = scripts.open_dataset(OPT, "rgb", OPT.height, OPT.width, ctx)                          # :69-73; rgb: converted with the generated half (:173-176)
    loop = None if OPT.compat else DeviceDistill(s)
    pictures = progress.DistillPictures(loop, OPT.save) if OPT.progress else None
    half, last, path, t0 = OPT.batchSize // 2, None, None, time.perf_counter()
    pull = (lambda: (s.G.pull_params(), s.D.pull_params())) if loop is None else loop.sync_to_host
    try:
        for i in range(1, OPT.N_batches + 1):                                                       # :161
            real = real_images(OPT, data, i, half, DATASET)
            want = not OPT.quiet or i == OPT.N_batches
            if loop is None:
                last = compat_batch(s, i, real)
            else:
                last = loop.batch(real, want_loss=want) or last
                if isinstance(real, nn_utils.DeviceTensor):
                    real.free()                                                                     # the batch's draw from the cache
            if not OPT.quiet:
                print("<batch %d of %d (%.2f%%)> loss G: %.4f, loss D: %.4f" % (i, OPT.N_batches, 100.0 * i / OPT.N_batches, last[0], last[1]))
            if pictures is not None and i % 10 == 0:                                                # :245-247
                pictures.visualize(picture_images(OPT, data, i, DATASET), i)
            if i % OPT.saveFreq == 0:                                                               # :249-251
                pull()
                path = save(OPT, s)
        pull()
        path = save(OPT, s)                                                                         # :257
        if not OPT.quiet:
            print("<trainer> %.1f images/s" % (OPT.N_batches * OPT.batchSize / (time.perf_counter() - t0)))
    finally:
        if pictures is not None:
            pictures.close()
        if loop is not None:
            loop.close()
    return dict(path=path, last_losses=last, G=s.G, D=s.D, state=s, pictures=pictures)


if __name__ == "__main__":
    main()
