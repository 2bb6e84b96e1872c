"""The pieces that turn pretrain_g's autoencoder into a variational one (new: the reference has no counterpart; its README lists "Compare to
Autoencoders, especially VAEs" first under further research).  The encoder head (models.create_VAE_encoder) emits h = (mu | logvar); the sampling
layer between encoder and decoder is gr_vae_sample_dev / gr_vae_sample_backward_dev (csrc/vae.hip; the arithmetic is stated in include/ganrev.h):

    z = mu + exp(logvar / 2) eps,    KL_i = sum_t 0.5 (mu^2 + exp(logvar) - 1 - logvar),    loss = recon + kl_weight mean_i KL_i

ganrev.train_vae trains the pair; what it saves are ordinary checkpoints: the decoder is a G, and mean_reverser(encoder) - the encoder cut to its
mu half - is an R, so `apply_r --G vae.net --R vae_r.net` runs the whole analysis on the VAE's latent space.
"""
import copy

from . import _lib as L
from . import nn


class Sample:
    """The sampling layer on host arrays (gr_vae_sample_host / gr_vae_sample_backward_host: the device kernels on staged copies, the same bits):
    what train_vae --compat puts between ae.forward / backward of the two nets.  forward keeps h and eps for backward, as an nn module keeps
    its input."""

    def __init__(self, ctx=None):
        self.ctx = ctx if ctx is not None else L.default_context()
        self.h = self.eps = self.output = self.kl_rows = self.kl = self.gradInput = None

    def forward(self, h, eps=None):
        """h [B x 2 nd], eps [B x nd] or None (eps = 0) -> z [B x nd]; kl_rows [B] and kl, their mean, stay on the layer"""
        self.h, self.eps = L.f32(h).copy(), None if eps is None else L.f32(eps).copy()
        self.output, self.kl_rows, self.kl = self.ctx.vae_sample_host(self.h, self.eps)
        return self.output

    def backward(self, gz, kl_weight):
        """gz = d recon / d z [B x nd] -> the gradient of recon + kl_weight mean_i KL_i with respect to h [B x 2 nd]"""
        if self.h is None:
            raise L.GanrevError("vae.Sample: backward called before forward")
        self.gradInput = self.ctx.vae_sample_backward_host(self.h, self.eps, gz, kl_weight)
        return self.gradInput


def mean_reverser(encoder):
    """An encoder (models.create_VAE_encoder, host parameters current: pull_params first) -> a new nn.Sequential image -> noiseDim that computes
    the mu half of the encoder: every leaf copied, BatchNorm running statistics included, the last nn.Linear cut to its first noiseDim output
    rows, weight and bias.  An ordinary net: t7.save_checkpoint(R=...) writes it and apply_r --R reads it."""
    leaves = encoder.leaves()
    if not leaves or not isinstance(leaves[-1], nn.Linear) or leaves[-1].weight.shape[0] % 2:
        raise L.GanrevError("mean_reverser: the encoder must end in an nn.Linear with 2 noiseDim outputs (mu | logvar)")
    R = nn.Sequential()
    for m in leaves[:-1]:
        c = copy.deepcopy(m)                       # its own arrays: parameters and running statistics
        if isinstance(c, nn._Param):
            c.gradWeight = c.gradBias = None
        R.add(c)
    head = leaves[-1]
    nd = head.weight.shape[0] // 2
    cut = nn.Linear(head.weight.shape[1], nd)
    cut.weight[...] = head.weight[:nd]
    cut.bias[...] = head.bias[:nd]
    R.add(cut)
    R.train = encoder.train
    for m in R.leaves():
        m.train = encoder.train
    return R


def encode(ctx, encoder_dev_model, images_dev, n, batch):
    """mu [n x noiseDim] and the KL of every row against the unit Gaussian [n] (host arrays) for the device table images_dev of n images:
    the encoder (a device.DeviceModel) in evaluate() mode in chunks of `batch`, then gr_vae_sample_dev with eps null, whose z is mu.  The KL is an
    anomaly score in the VAE's own terms: how far the posterior of an image lies from the prior.  The nets return to the mode they were in."""
    enc = encoder_dev_model
    n, batch = int(n), int(batch)
    feat, width = enc.in_features(enc.model), enc.out_features(enc.model)
    if width % 2 or width // 2 > ctx.VAE_MAX_ND:
        raise L.GanrevError(f"vae.encode: the encoder emits {width} features: (mu | logvar) of at most {ctx.VAE_MAX_ND} dimensions each")
    nd = width // 2
    modes = [net.training for net in enc.nets]
    mu_dev = ctx.malloc(4 * n * nd)
    kl_dev = ctx.malloc(4 * n)
    try:
        enc.set_training(False)
        for lo in range(0, n, batch):
            b = min(batch, n - lo)
            h = enc.forward(images_dev + 4 * feat * lo, b)
            ctx.vae_sample_dev(h, None, b, nd, mu_dev + 4 * nd * lo, kl_dev + 4 * lo, None)
        return ctx.download(mu_dev, (n, nd)), ctx.download(kl_dev, (n,))
    finally:
        for net, t in zip(enc.nets, modes):
            net.set_training(t)
        ctx.free(mu_dev)
        ctx.free(kl_dev)
