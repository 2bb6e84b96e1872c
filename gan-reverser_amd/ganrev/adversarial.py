"""Mirror of the reference's GAN game, adversarial.lua:1-205 (driven by train.lua:125-330) - SURVEY.md 8f rank 4.

adversarial.train(env, trainData) plays one epoch: per batch, D is updated on half a batch of real and half a batch of
generated images (fevalD, adversarial.lua:66-100), then G is updated through D (fevalG_on_D, adversarial.lua:104-133: G forward,
D forward, BCE against "real", D backward to the images, G backward from D's gradInput).  The reference keeps its state in Lua
globals (OPT, MODEL_D, MODEL_G, CRITERION, PARAMETERS_*, GRAD_PARAMETERS_*, OPTSTATE, CONFUSION, EPOCH ...); here the same
names live on one `env` object (make_env builds it the way train.lua:125-200 does).

Everything numeric runs on the GPU through libganrev.so: G and the compiled parts of D (ganrev.nn), nn.BCECriterion
(gr_bce_host), optim.adam (gr_adam_step).  The penalty / clamp lines are host numpy on the flat vectors, as they are Torch
tensor ops on the host-visible flat vectors in the reference.
"""
import types

import numpy as np

from . import _lib as L
from . import device, nn, nn_utils, optim

Y_GENERATOR = 0          # train.lua:67-68
Y_NOT_GENERATOR = 1


def clamp(gradParameters, clampValue):
    """adversarial.lua:8-12"""
    if clampValue != 0:
        np.clip(gradParameters, -clampValue, clampValue, out=gradParameters)


def l1(parameters, gradParameters, lossValue, l1weight):
    """adversarial.lua:14-20.  The reference misspells its own argument in the gradient line (`l1Weight`, a nil global), so a
    non-zero weight raises there; every shipped configuration has L1 = 0 (train.lua:29,31).  Implemented as evidently meant."""
    if l1weight != 0:
        lossValue = lossValue + l1weight * float(np.abs(parameters).sum(dtype=np.float64))
        gradParameters += np.sign(parameters) * np.float32(l1weight)
    return lossValue


def l2(parameters, gradParameters, lossValue, l2weight):
    """adversarial.lua:22-28"""
    if l2weight != 0:
        lossValue = lossValue + l2weight * float(np.dot(parameters.astype(np.float64), parameters.astype(np.float64))) / 2
        gradParameters += parameters * np.float32(l2weight)
    return lossValue


def penalise_and_clamp(parameters, gradParameters, lossValue, l1weight, l2weight, clampValue):
    """adversarial.lua:86-88, and the `penalties (L1 and L2)` / `clamp` lines of every other --compat closure (train_r.lua:153-165,
    pretrain_g.lua:162-175, pretrain_with_previous_net.lua:196-208,224-236) -> the penalised loss value"""
    lossValue = l1(parameters, gradParameters, lossValue, l1weight)
    lossValue = l2(parameters, gradParameters, lossValue, l2weight)
    clamp(gradParameters, clampValue)
    return lossValue


def make_env(MODEL_G, MODEL_D, IMG_DIMENSIONS, **opt):
    """The globals train.lua:125-200 sets up, with its option defaults (train.lua:27-38)."""
    OPT = types.SimpleNamespace(batchSize=32, N_epoch=30, noiseDim=100, noiseMethod="normal", G_L1=0.0, G_L2=0.0, D_L1=0.0, D_L2=1e-4,
                                D_iterations=1, G_iterations=1, D_clamp=1.0, G_clamp=5.0, D_optmethod="adam", G_optmethod="adam", seed=1,
                                D_sgd_lr=0.02, G_sgd_lr=0.02, D_sgd_momentum=0.0, G_sgd_momentum=0.0)
    for k, v in opt.items():
        if not hasattr(OPT, k):
            raise L.GanrevError(f"unknown option '{k}'")
        setattr(OPT, k, v)
    env = types.SimpleNamespace(OPT=OPT, MODEL_G=MODEL_G, MODEL_D=MODEL_D, IMG_DIMENSIONS=tuple(IMG_DIMENSIONS), EPOCH=1,
                                Y_GENERATOR=Y_GENERATOR, Y_NOT_GENERATOR=Y_NOT_GENERATOR)
    env.CRITERION = nn.BCECriterion()                                           # train.lua:173
    env.PARAMETERS_D, env.GRAD_PARAMETERS_D = MODEL_D.getParameters()           # train.lua:176-177
    env.PARAMETERS_G, env.GRAD_PARAMETERS_G = MODEL_G.getParameters()
    env.CONFUSION = np.zeros((2, 2), np.int64)                                  # train.lua:180 optim.ConfusionMatrix: [predicted][target]
    env.OPTSTATE = {k: {"D": {}, "G": {}} for k in ("adagrad", "adadelta", "adamax", "adam", "rmsprop")}      # train.lua:183-193
    env.OPTSTATE["sgd"] = {"D": {"learningRate": OPT.D_sgd_lr, "momentum": OPT.D_sgd_momentum},
                           "G": {"learningRate": OPT.G_sgd_lr, "momentum": OPT.G_sgd_momentum}}
    env.noise_counter = 0
    MODEL_D.training(); MODEL_G.training()                                      # train.lua:133-134
    return env


def _noise(env, N):
    env.noise_counter += 1
    return nn_utils.createNoiseInputs(N, env.OPT.noiseDim, env.OPT.noiseMethod, seed=env.OPT.seed * 100003 + env.noise_counter)


def createImages(env, N):
    """NN_UTILS.createImages(N, false) (utils/nn_utils.lua:57-89): MODEL_G:forward on fresh noise, OPT.batchSize rows at a time."""
    noise = _noise(env, N)
    out = None
    for lo in range(0, N, env.OPT.batchSize):
        gen = env.MODEL_G.forward(noise[lo:lo + env.OPT.batchSize]).copy()
        if out is None:
            out = np.empty((N,) + gen.shape[1:], np.float32)
        out[lo:lo + gen.shape[0]] = gen
    return out


def make_fevalD(env, inputs, targets):
    """adversarial.lua:66-100: f(X) and df/dX of the discriminator on the batch (inputs, targets)."""
    def fevalD(x):
        if x is not env.PARAMETERS_D:
            env.PARAMETERS_D[...] = x
        env.GRAD_PARAMETERS_D[...] = 0                                          # :74
        outputs = env.MODEL_D.forward(inputs)                                   # :79
        f = env.CRITERION.forward(outputs, targets.reshape(outputs.shape))      # :80
        df_do = env.CRITERION.backward(outputs, targets.reshape(outputs.shape)) # :83
        env.MODEL_D.backward(inputs, df_do)                                     # :84
        f = penalise_and_clamp(env.PARAMETERS_D, env.GRAD_PARAMETERS_D, f, env.OPT.D_L1, env.OPT.D_L2, env.OPT.D_clamp)      # :86-88
        for i in range(outputs.shape[0]):                                       # :91-96
            c = 1 if outputs[i][0] > 0.5 else 0
            env.CONFUSION[c, int(targets[i])] += 1
        return f, env.GRAD_PARAMETERS_D
    return fevalD


def make_fevalG_on_D(env, noiseInputs, targets):
    """adversarial.lua:104-133: f(X) and df/dX of the generator, rated by D."""
    def fevalG_on_D(x):
        if x is not env.PARAMETERS_G:
            env.PARAMETERS_G[...] = x
        env.GRAD_PARAMETERS_G[...] = 0                                          # :110
        samples = env.MODEL_G.forward(noiseInputs).copy()                       # :113
        outputs = env.MODEL_D.forward(samples)                                  # :114
        f = env.CRITERION.forward(outputs, targets.reshape(outputs.shape))      # :115
        df_samples = env.CRITERION.backward(outputs, targets.reshape(outputs.shape))   # :119
        env.MODEL_D.backward(samples, df_samples)                               # :120
        df_do = env.MODEL_D.gradInput                                           # :121  MODEL_D.modules[1].gradInput
        env.MODEL_G.backward(noiseInputs, df_do)                                # :124
        f = penalise_and_clamp(env.PARAMETERS_G, env.GRAD_PARAMETERS_G, f, env.OPT.G_L1, env.OPT.G_L2, env.OPT.G_clamp)      # :126-128
        return f, env.GRAD_PARAMETERS_G
    return fevalG_on_D


def _optimize(env, which, feval, params, model):
    """adversarial.lua:156-171 / 183-198: the optimiser chosen with --D_optmethod / --G_optmethod on the host flat vectors.  adam (the
    default) updates through the fused device kernel; the other five are host mirrors of the optim rock (ganrev/optim.py) here, in the
    --compat game - DeviceGame steps them on the device with gr_optim_step."""
    method = getattr(env.OPT, which + "_optmethod")
    if method == "adam":
        return optim.adam(feval, params, env.OPTSTATE["adam"][which], model=model)
    if method not in optim.METHODS:
        raise L.GanrevError(f"Unknown optimizer method '{method}' chosen for {which}.")        # adversarial.lua:170, 197
    return optim.METHODS[method](feval, params, env.OPTSTATE[method][which])      # the host vector is authoritative: the next forward uploads it


def train(env, trainData, quiet=True):
    """adversarial.lua:37-205.  trainData: [N x C x H x W] real images; N >= N_epoch * batchSize/2 * D_iterations (train.lua:214)."""
    OPT = env.OPT
    batchSize, batchesPerEpoch = OPT.batchSize, OPT.N_epoch
    if batchesPerEpoch <= 0:
        batchesPerEpoch = 100                                                   # :42
    exampleForDIdx = 0
    nbExamplesD = nbExamplesG = 0
    losses = {"D": [], "G": []}
    if not quiet:
        print("<trainer> Epoch #%d [batchSize = %d]" % (env.EPOCH, batchSize))
    for batchIdx in range(1, batchesPerEpoch + 1):
        inputs = np.empty((batchSize,) + env.IMG_DIMENSIONS, np.float32)        # :54-56
        targets = np.empty(batchSize, np.float32)
        for _ in range(OPT.D_iterations):                                       # (1) update D  :139-174
            half = batchSize // 2
            if exampleForDIdx + half > len(trainData):
                raise IndexError("trainData exhausted (adversarial.lua:146 indexes past the loaded examples)")
            inputs[:half] = trainData[exampleForDIdx:exampleForDIdx + half]     # :141-149
            targets[:half] = env.Y_NOT_GENERATOR
            exampleForDIdx += half
            inputs[half:2 * half] = createImages(env, half)                     # :152-157
            targets[half:2 * half] = env.Y_GENERATOR
            _, fs = _optimize(env, "D", make_fevalD(env, inputs, targets), env.PARAMETERS_D, env.MODEL_D)
            losses["D"].append(fs[0])
            nbExamplesD += inputs.shape[0]
        for _ in range(OPT.G_iterations):                                       # (2) update G  :178-201
            noiseInputs = _noise(env, batchSize)
            targets[...] = env.Y_NOT_GENERATOR
            _, fs = _optimize(env, "G", make_fevalG_on_D(env, noiseInputs, targets), env.PARAMETERS_G, env.MODEL_G)
            losses["G"].append(fs[0])
            nbExamplesG += noiseInputs.shape[0]
    if not quiet:
        print("Trained G on: %d | Trained D on: %d" % (nbExamplesG, nbExamplesD))
        print(env.CONFUSION)
    tV = float(np.trace(env.CONFUSION)) / max(1, int(env.CONFUSION.sum()))     # :201 CONFUSION.totalValid
    env.CONFUSION[...] = 0
    env.last_losses = losses
    return tV


# ---------------------------------------------------------------------------------------------------------------------
# Fast mode: the same game with images, gradients, parameters and the optimiser state resident on the GPU (what ganrev.train_r's
# DeviceTrainer / gr_train_r_step is to train_r.lua:138-170).  G and D each run through a device.DeviceModel, nn.BCECriterion is
# gr_bce_dev, and adversarial.l1 / l2 / clamp + the optimiser chosen for the net (train.lua:37-38) are one fused launch per part:
# gr_adam_step for adam, gr_optim_step for sgd, adagrad, adadelta, adamax and rmsprop.  Nothing is copied to the host inside a batch
# except, on request, the two loss values.
class DeviceGame:
    """adversarial.lua:139-201 per batch, device-resident.  game = DeviceGame(env); game.batch(real_half_batch) per batch;
    game.sync_to_host() before anything reads env.PARAMETERS_* or the host-side modules again (save, evaluate, compat mode)."""

    def __init__(self, env):
        self.env = env
        OPT, G, D = env.OPT, env.MODEL_G, env.MODEL_D
        for which in ("D", "G"):
            method = getattr(OPT, which + "_optmethod")
            if method != "adam" and method not in L.OPT_METHODS:
                raise L.GanrevError(f"Unknown optimizer method '{method}' chosen for {which}.")        # adversarial.lua:170, 197
        self.ctx = ctx = G._context()
        B = OPT.batchSize
        device.compile_models(nn_utils.createNoiseInputs(2, OPT.noiseDim, OPT.noiseMethod, seed=1), G, D)
        self.gg, self.dg = device.DeviceModel(ctx, G), device.DeviceModel(ctx, D)
        self.gnet = G._net                                  # G's one net by name: not used by the game, read by tools/debug
        for m in (self.gg, self.dg):
            m.set_training(True)
            m.adam_reset()                                  # the two state vectors of every part, whichever method steps it (= optim_reset)
        self.t = {"D": 0, "G": 0}
        self.npix = int(np.prod(env.IMG_DIMENSIONS))
        self.mem = device.Buffers(ctx)
        m = self.mem.malloc
        self.inputs, self.targets, self.ones = m(4 * B * self.npix), m(4 * B), m(4 * B)
        self.noise, self.df, self.loss = m(4 * B * OPT.noiseDim), m(4 * B), m(16)
        half = B // 2
        ctx.upload(np.concatenate([np.full(half, Y_NOT_GENERATOR, np.float32), np.full(B - half, Y_GENERATOR, np.float32)]), self.targets)
        ctx.upload(np.full(B, Y_NOT_GENERATOR, np.float32), self.ones)
        self.hyper_d = self._config("D", OPT.D_L1, OPT.D_L2, OPT.D_clamp)
        self.hyper_g = self._config("G", OPT.G_L1, OPT.G_L2, OPT.G_clamp)
        self.noise_counter = self.batches = 0

    def _config(self, which, l1, l2, clamp):
        """adversarial.lua:147-161 / 174-188: adam's gr_hyper, or the gr_optim_config of the method chosen for this net, read from the table
        train.lua:183-193 gives it (OPTSTATE.sgd carries learningRate and momentum; the other tables are empty: the rock's defaults)"""
        method = getattr(self.env.OPT, which + "_optmethod")
        if method == "adam":
            return L.Hyper(l1=l1, l2=l2, clamp=clamp)
        return L.OptimConfig(method, self.env.OPTSTATE[method][which], l1=l1, l2=l2, clamp=clamp)

    def _step(self, which, model, config):
        """optim[method](feval, PARAMETERS, OPTSTATE[method][which]) once the closure's gradient is in place: one fused launch per part"""
        self.t[which] += 1
        if isinstance(config, L.Hyper):
            model.adam_step(config, self.t[which])
        else:
            model.optim_step(config, self.t[which])

    def _fill_noise(self, N, host=None):
        OPT = self.env.OPT
        if host is None:
            self.noise_counter += 1
        self.ctx.fill_noise(self.noise, N * OPT.noiseDim, OPT.noiseMethod, OPT.seed * 100003 + self.noise_counter, host)

    def batch(self, real, noise_d=None, noise_g=None, want_loss=False):
        """One batch of adversarial.lua:139-201: OPT.D_iterations updates of D, each on batchSize/2 fresh real images + batchSize/2
        generated ones, then OPT.G_iterations updates of G through D.  real: [D_iterations * batchSize/2 x C x H x W] host array (the
        one upload), or a nn_utils.DeviceTensor of that shape (a draw from the dataset cache), copied where it lies.  noise_*: host noise to use instead of device-generated noise (parity tests): arrays of
        [D_iterations * batchSize/2 x noiseDim] / [G_iterations * batchSize x noiseDim].  Returns the LAST (loss_D, loss_G)."""
        OPT, B = self.env.OPT, self.env.OPT.batchSize
        half = B // 2
        ctx, gg, dg = self.ctx, self.gg, self.dg
        # `for k=1,OPT.D_iterations` (adversarial.lua:127,168): 0 iterations run zero times - that phase's net stays frozen
        nD, nG = max(0, int(OPT.D_iterations)), max(0, int(OPT.G_iterations))
        on_device = isinstance(real, nn_utils.DeviceTensor)
        if on_device and real.size != real.shape[0] * self.npix:
            raise L.GanrevError(f"DeviceGame.batch: device images {real.shape} are not [n x {self.npix} values]")
        if not on_device:
            real = np.ascontiguousarray(real, np.float32).reshape(-1, self.npix)
        if real.shape[0] < nD * half:
            raise IndexError("trainData exhausted (adversarial.lua:146 indexes past the loaded examples): "
                             f"{real.shape[0]} images for {nD} D iterations of {half}")
        self.batches += 1
        device.range_guard(ctx, self.batches, (gg, dg))
        loss_d = loss_g = None
        for k in range(nD):
            # (1) D on half real, half generated (adversarial.lua:141-157, fevalD :66-100)
            if on_device:
                ctx.copy2d(self.inputs, self.npix, real.ptr + 4 * k * half * self.npix, self.npix, half, self.npix)
            else:
                ctx.upload(real[k * half:(k + 1) * half], self.inputs)
            self._fill_noise(half, None if noise_d is None else np.asarray(noise_d).reshape(nD, half, -1)[k])
            fake = gg.forward(self.noise, half)
            ctx.copy2d(self.inputs + 4 * half * self.npix, self.npix, fake, self.npix, half, self.npix)
            dg.zero_grads()
            out = dg.forward(self.inputs, B)
            ctx.bce_dev(out, self.targets, B, self.loss, self.df)
            dg.backward(self.df, B, False)
            self._step("D", dg, self.hyper_d)
            if want_loss and k == nD - 1:
                loss_d = ctx.read_loss(self.loss)
        for k in range(nG):
            # (2) G through D (adversarial.lua:178-201, fevalG_on_D :104-133)
            self._fill_noise(B, None if noise_g is None else np.asarray(noise_g).reshape(nG, B, -1)[k])
            gg.zero_grads()
            samples = gg.forward(self.noise, B)
            out = dg.forward(samples, B)
            ctx.bce_dev(out, self.ones, B, self.loss, self.df)
            df_do = dg.backward(self.df, B, True)
            gg.backward(df_do, B, False)
            self._step("G", gg, self.hyper_g)
            if want_loss and k == nG - 1:
                loss_g = ctx.read_loss(self.loss)
        return loss_d, loss_g

    def sync_to_host(self):
        """Parameters and BatchNorm statistics into the host modules; for a net stepped by one of the five other methods also its state into
        env.OPTSTATE[method][which] under the keys the mirror in ganrev/optim.py keeps it (dfdx, evalCounter | paramVariance, accDelta | m, u, t), so
        that adversarial.train continues from it.  (adam's moments stay on the device, as before: optim.adam re-uploads what its table holds.)"""
        self.env.MODEL_D.pull_params()
        self.env.MODEL_G.pull_params()
        for which, model, config in (("D", self.dg, self.hyper_d), ("G", self.gg, self.hyper_g)):
            if isinstance(config, L.Hyper) or self.t[which] == 0:
                continue                                    # a net no step has touched keeps the table train.lua gave it
            method = getattr(self.env.OPT, which + "_optmethod")
            state = self.env.OPTSTATE[method][which]
            for key, used, vec in zip(L.OPT_STATE_KEYS[method], config.slots(), model.optim_state()):
                if key is not None and used:
                    state[key] = vec
            if method == "adamax":
                state["t"] = self.t[which]
            elif method != "rmsprop":
                state["evalCounter"] = self.t[which]

    def close(self):
        """Release the device buffers of the game (the nets stay with their models)."""
        for m in (self.gg, self.dg, self.mem):
            m.close()
