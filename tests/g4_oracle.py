"""Oracle twin of a create_G4-shaped model (reference models.lua:145-194): an nn.Concat(2) of structurally identical branches
(Linear - PReLU - Linear - BatchNorm - PReLU - Reshape - up-sampling - 3x3 convolution - BatchNorm - PReLU) and a convolutional tail.
The oracle's go_net is a plain nn.Sequential, so the twin - always built from a model on the parts route
(`concat.bundle = False`: the oracle never sees a grouped kind) - is one oracle net per branch and one for the tail, each built from layer kinds
the oracle has always evaluated, joined in numpy the way nn.Concat joins its branches (helpers.OracleGraph's rule): channel
concatenation forward, channel slices and the float32 sum of the branches' gradInputs backward.  Also the miniature model the GPU tests
train on, and the conditioning test they choose their input seed with."""
import numpy as np

from helpers import OracleGraph

KINK_GAP = 1e-4          # no pre-activation feeding an nn.PReLU may lie this close to zero: its derivative flips there
SEEDS = range(1, 41)     # the input seeds pick_seed searches, in this order


def mini_g4(nb=3, nd=5, hidden=4, planes=2, side=4, tail=4, channels=1, seed=11, bundle=True):
    """create_G4 in small: nb branches Linear(nd, hidden) - PReLU - Linear(hidden, planes * side * side) - BatchNorm - PReLU -
    Reshape(planes, side, side) - up-sampling - conv(planes, planes) - BatchNorm - PReLU, then conv(nb * planes, tail) - BatchNorm -
    PReLU - conv(tail, channels) - Sigmoid.  Every parameter and running statistic is drawn (synth.init_params), every slope its own.
    bundle = False keeps the parts route (nb branch nets and a tail net); the parameters are the same either way."""
    from ganrev import models, nn, synth
    nn.manualSeed(seed)
    model = nn.Sequential()
    concat = nn.Concat(2)
    if not bundle:
        concat.bundle = False
    for _ in range(nb):
        seq = nn.Sequential()
        seq.add(nn.Linear(nd, hidden))
        seq.add(nn.PReLU())
        seq.add(nn.Linear(hidden, planes * side * side))
        seq.add(nn.BatchNormalization(planes * side * side))
        seq.add(nn.PReLU())
        seq.add(nn.Reshape(planes, side, side))
        seq.add(nn.SpatialUpSamplingNearest(2))
        seq.add(models._CudnnSpatialConvolution(planes, planes, 3, 3, 1, 1, 1, 1))
        seq.add(nn.SpatialBatchNormalization(planes))
        seq.add(nn.PReLU())
        concat.add(seq)
    model.add(concat)
    model.add(models._CudnnSpatialConvolution(nb * planes, tail, 3, 3, 1, 1, 1, 1))
    model.add(nn.SpatialBatchNormalization(tail))
    model.add(nn.PReLU())
    model.add(models._CudnnSpatialConvolution(tail, channels, 3, 3, 1, 1, 1, 1))
    model.add(nn.Sigmoid())
    synth.init_params(model, seed)
    rng = np.random.default_rng(seed)
    for m in model.leaves():
        if m.typename == "nn.PReLU":
            m.weight[...] = rng.uniform(0.1, 0.4)           # not 32 copies of 0.25: a slope landing in the wrong place must show
    return model


class G4Oracle(OracleGraph):
    """helpers.OracleGraph (one oracle net per compiled chunk, nn.Concat joined in numpy) with what the G4 tests also need: the flat
    parameter vector in getParameters() order, the PReLU conditioning of the last forward, the BatchNorm running statistics per
    module and the oracle's Adam step on the flat vectors."""

    @property
    def params(self):
        return np.concatenate([o.params for _, o in self.pairs])

    def set_params(self, flat):
        lo = 0
        for _, o in self.pairs:
            o.params[...] = flat[lo:lo + o.params.size]
            lo += o.params.size

    def min_kink_distance(self):
        """smallest |input| over every nn.PReLU of the last forward"""
        best = np.inf
        for chunk, onet in self.pairs:
            for m in chunk.leaves():
                if m.typename == "nn.PReLU":
                    li = onet.layer_index[id(m)]
                    assert li > 0, "a PReLU opens a chunk: its input is not a layer output"
                    best = min(best, float(np.abs(onet.layer_output(li - 1)).min()))
        return best

    def bn_running(self):
        """[(module, running_mean, running_var)] of every BatchNorm module, in tree order"""
        out = []
        for chunk, onet in self.pairs:
            bi = 0
            for m in chunk.leaves():
                if hasattr(m, "running_mean"):
                    rm, rv = onet.bn_running(bi)
                    out.append((m, np.array(rm, copy=True), np.array(rv, copy=True)))
                    bi += 1
        return out

    def adam_step(self, oracle, hyper, t, m, v):
        """penalty, clamp and optim.adam on the flat vectors (element-wise, so the chunk boundaries do not matter) -> new parameters"""
        theta, g = self.params.copy(), self.grads.copy()
        oracle.penalty_clamp_adam(theta, g, m, v, hyper, t)
        self.set_params(theta)
        return theta


def pick_seed(og, shape, training):
    """The first input seed of SEEDS whose oracle forward keeps every PReLU input KINK_GAP away from zero (two correct fp32 forwards may
    sit on different sides of a kink closer than their rounding, and the PReLU derivative differs there) -> (seed, x, oracle output)."""
    from ganrev import synth
    og.set_training(training)
    for seed in SEEDS:
        x = synth.normal(shape, seed)
        ref = og.forward(x)
        if og.min_kink_distance() >= KINK_GAP:
            return seed, x, ref
    raise AssertionError(f"no input seed in {SEEDS.start}..{SEEDS.stop - 1} keeps every PReLU input {KINK_GAP:g} away from zero")


# ---------------------------------------------------------------------------------------------------------------- the single kinds
def torch_reference(descs, dims, params, x, gout):
    """A layer-descriptor list (kind, a, b, c, p, flags) in float64 PyTorch, training mode: the oracle of the grouped kinds alone and of
    the short chains they are tested in.  Kinds: LINEAR, GROUPLINEAR, CONV3, GROUPCONV3, CONVK, UPSAMPLE2, BN (batch statistics, eps 1e-5), PRELU
    (a = n slopes), VIEW, SIGMOID.  params: the flat vector in layer order (weight, bias | gamma, beta | slopes).
    -> dict(out, gin, grads, kink = smallest |PReLU input|, segs = [(layer, name, lo, hi, in front of a BatchNorm)])"""
    import torch
    import torch.nn.functional as F
    import ganrev._lib as L
    theta = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    xin = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    h = xin.reshape((x.shape[0],) + tuple(dims))
    off, segs, kink = 0, [], np.inf

    def take(n, shape, layer, name, before_bn=False):
        nonlocal off
        t = theta[off:off + n].reshape(shape)
        segs.append((layer, name, off, off + n, before_bn))
        off += n
        return t
    for i, (kind, a, b, c, _, _) in enumerate(descs):
        nxt_bn = i + 1 < len(descs) and descs[i + 1][0] == L.BN
        B = h.shape[0]
        if kind in (L.LINEAR, L.GROUPLINEAR):
            G = c if kind == L.GROUPLINEAR else 1
            w, bias = take(b * (a // G), (G, b // G, a // G), i, "weight"), take(b, (b,), i, "bias", nxt_bn)
            h = torch.einsum("bgk,gmk->bgm", h.reshape(B, G, a // G), w).reshape(B, b) + bias
            h = h.reshape(B, b, 1, 1)
        elif kind in (L.CONV3, L.GROUPCONV3):
            G = c if kind == L.GROUPCONV3 else 1
            w, bias = take(b * (a // G) * 9, (b, a // G, 3, 3), i, "weight"), take(b, (b,), i, "bias", nxt_bn)
            h = F.conv2d(h, w, bias, padding=1, groups=G)
        elif kind == L.CONVK:                   # c = the odd window K (tests/generic_paths.py: 1 and 5), padding (K - 1) / 2
            w, bias = take(b * a * c * c, (b, a, c, c), i, "weight"), take(b, (b,), i, "bias", nxt_bn)
            h = F.conv2d(h, w, bias, padding=c // 2)
        elif kind == L.UPSAMPLE2:
            h = h.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        elif kind == L.BN:
            gamma, beta = take(a, (a,), i, "weight"), take(a, (a,), i, "bias")
            h = F.batch_norm(h, None, None, gamma, beta, True, 0.1, 1e-5)
        elif kind == L.PRELU:
            n = a if a >= 2 else 1
            w = take(n, (n,), i, "weight")
            kink = min(kink, float(h.detach().abs().min()))
            h = torch.where(h > 0, h, w.repeat_interleave(h.shape[1] // n).reshape(1, -1, 1, 1) * h)
        elif kind == L.VIEW:
            h = h.reshape(B, a, max(b, 1), max(c, 1))
        elif kind == L.SIGMOID:
            h = torch.sigmoid(h)
        else:
            raise ValueError(f"torch_reference: kind {kind}")
    assert off == theta.numel(), (off, theta.numel())
    h.backward(torch.tensor(np.asarray(gout, np.float64)).reshape(h.shape))
    return dict(out=h.detach().numpy(), gin=xin.grad.numpy().reshape(x.shape), grads=theta.grad.numpy(), kink=kink, segs=segs)


def assert_segments_close(got, ref, segs, what, rtol=1e-4, floor=1e-3):
    """helpers.assert_grads_close's rule on explicit segments: every tensor within rtol of the largest reference gradient entry of ITS
    layer (floor 1e-3); a bias in front of a BatchNorm has an exactly-zero true gradient and must be rounding residue on both sides."""
    layer_max = {}
    for layer, _, lo, hi, _ in segs:
        layer_max[layer] = max(layer_max.get(layer, 0.0), float(np.abs(ref[lo:hi]).max()))
    for layer, name, lo, hi, before_bn in segs:
        gmax = max(layer_max[layer], floor)
        if name == "bias" and before_bn:
            assert float(np.abs(got[lo:hi]).max()) <= 1e-3 * gmax and float(np.abs(ref[lo:hi]).max()) <= 1e-3 * gmax, f"{what} layer {layer} bias in front of BatchNorm is not residue"
            continue
        d = float(np.abs(got[lo:hi] - ref[lo:hi]).max())
        assert d <= rtol * gmax, f"{what} layer {layer} {name} [{lo}:{hi}]: max |diff| {d:.3e} vs layer max |g| {gmax:.3e}"
