"""Oracle twin of a model that holds nn.SpatialAveragePooling(2,2,2,2) layers.  The C oracle has no such layer kind, so the
model is split at every average pool: each run of other layers is one oracle.Net, and between them the pool runs here in
numpy float32 with THNN's arithmetic (sum = 0, the window added in scan order, then / 4; backward: every window element
receives gradOutput / 4).  Modelled on helpers.OracleGraph."""
import numpy as np

from ganrev import nn


def avgpool_forward(x):
    """THNN SpatialAveragePooling(2,2,2,2) in float32: floor mode (an odd last row / column is dropped)"""
    x = np.asarray(x, np.float32)
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2)
    s = np.zeros((B, C, Ho, Wo), np.float32)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        s = s + v[:, :, :, dy, :, dx]
    return s / np.float32(4)


def avgpool_backward(g, in_shape):
    g = np.asarray(g, np.float32) / np.float32(4)
    B, C, H, W = in_shape
    Ho, Wo = H // 2, W // 2
    out = np.zeros(in_shape, np.float32)
    out[:, :, :2 * Ho, :2 * Wo] = np.repeat(np.repeat(g, 2, axis=2), 2, axis=3)
    return out


class SplitOracle:
    """parts: ("net", leaves, oracle.Net) or ("avg", module); `layer` maps a leaf to (part net, its layer index there) and
    `dev_layer` to its layer index in the whole compiled gr_net"""

    def __init__(self, oracle, model, in_dims):
        self.model, self.parts, self.where = model, [], {}
        _, self.dev_index = model._descs(tuple(in_dims))
        run, dims = [], tuple(in_dims)
        self.in_dims = {}
        d = dims
        for m in model.leaves():
            self.in_dims[id(m)] = d
            _, d = m.desc(d)
        for m in model.leaves() + [None]:
            if m is None or m.typename == "nn.SpatialAveragePooling":
                if run:
                    seq = nn.Sequential()
                    for r in run:
                        seq.add(r)
                    onet = oracle.from_model(seq, dims)
                    for r in run:
                        self.where[id(r)] = (onet, onet.layer_index[id(r)])
                    self.parts.append(("net", run, onet))
                    for r in run:
                        _, dims = r.desc(dims)
                    run = []
                if m is not None:
                    self.parts.append(("avg", m))
                    _, dims = m.desc(dims)
            else:
                run.append(m)
        self.out_dims = dims
        self.nets = [p[2] for p in self.parts if p[0] == "net"]

    def dev_layer(self, m):
        return self.dev_index[id(m)]

    def set_training(self, t):
        for o in self.nets:
            o.set_training(t)

    def zero_grads(self):
        for o in self.nets:
            o.zero_grads()

    def set_mask(self, m, keep):
        onet, li = self.where[id(m)]
        onet.set_mask(li, keep)

    def mask_size(self, m, B):
        onet, li = self.where[id(m)]
        return onet.mask_size(li, B)

    @property
    def grads(self):
        g = [o.grads for o in self.nets]
        return np.concatenate(g) if g else np.zeros(0, np.float32)

    @property
    def params(self):
        return np.concatenate([o.params for o in self.nets])

    def bn_running(self):
        return [o.bn_running(i) for o in self.nets for i in range(o.n_bn())]

    def forward(self, x):
        x = np.ascontiguousarray(x, np.float32)
        self.inputs = []
        for p in self.parts:
            self.inputs.append(x)
            x = np.array(p[2].forward(x), copy=True) if p[0] == "net" else avgpool_forward(x)
        return x

    def backward(self, gout):
        g = np.ascontiguousarray(gout, np.float32)
        for p, x in zip(reversed(self.parts), reversed(self.inputs)):
            g = np.array(p[2].backward(x, g), copy=True) if p[0] == "net" else avgpool_backward(g, x.shape)
        return g

    def layer_output(self, m):
        onet, li = self.where[id(m)]
        return onet.layer_output(li)


def inject_masks(model, so, B, seed):
    """the same keep flags into the device net (whole-net layer) and the oracle part that holds the dropout"""
    from ganrev import synth
    for m in model.leaves():
        if m.typename in ("nn.Dropout", "nn.SpatialDropout"):
            n = so.mask_size(m, B)
            keep = synth.bernoulli_keep((n,), seed * 131 + so.dev_layer(m), m.p)
            so.set_mask(m, keep)
            model.setNoise(m, keep)


def adopt_device_choices(model, so, B, max_flips, near_tie=1e-4, rel_flips=0.0):
    """helpers.adopt_device_argmax / adopt_device_kinks for a split oracle: the device's max-pool argmax (read with the whole-net
    layer index) and the side of zero its ReLU / PReLU inputs took are forced onto the oracle part that holds the layer, after
    checking that the differences are few (max_flips, or rel_flips of the layer's elements when that is more) and rounding-level.
    Returns (argmax flips, kink flips)."""
    import ganrev._lib as L
    leaves = model.leaves()
    pflips, kflips = [], []
    for i, m in enumerate(leaves):
        if m.typename == "nn.SpatialMaxPooling":
            onet, li = so.where[id(m)]
            x = onet.layer_output(li - 1)
            ora = onet.pool_index(li)
            dev = model._net.pool_index(so.dev_layer(m), ora.size)
            diff = np.nonzero(dev != ora)[0]
            if diff.size:                  # a legitimate flip is a near-tie of the oracle's own window values
                c, h, w = so.in_dims[id(m)]
                win = x.reshape(-1, h // 2, 2, w // 2, 2).transpose(0, 1, 3, 2, 4).reshape(-1, 4).astype(np.float64)
                gap = win[diff, ora[diff]] - win[diff, dev[diff]]
                assert np.all(gap >= 0) and gap.max() < near_tie, f"max-pool layer {so.dev_layer(m)}: argmax gap {gap.max():.3e}"
            assert diff.size <= max_flips, f"max-pool layer {so.dev_layer(m)}: {diff.size} of {ora.size} windows differ in argmax"
            onet.force_pool_index(li, dev)
            pflips.append(int(diff.size))
        elif m.typename in ("nn.ReLU", "cudnn.ReLU", "nn.PReLU"):
            onet, li = so.where[id(m)]
            z = onet.layer_output(li - 1)
            own = z > 0
            nxt = leaves[i + 1].typename if i + 1 < len(leaves) else ""
            lj = so.dev_layer(m) + (1 if nxt in ("nn.Dropout", "nn.SpatialDropout") and m.typename != "nn.PReLU" else 0)
            try:
                dev = model._net.layer_output(lj, (z.size,))
            except L.GanrevError:
                continue                   # fused into its stage (a pool follows): the device keeps no copy to read the side from
            side = np.where(dev != 0, dev > 0, own if m.typename == "nn.PReLU" or lj != so.dev_layer(m) else False)
            diff = np.nonzero(side != own)[0]
            if diff.size:
                assert np.abs(z[diff]).max() < near_tie, f"activation layer {so.dev_layer(m)}: |input| {np.abs(z[diff]).max():.3e} is not rounding-level"
            assert diff.size <= max(max_flips, rel_flips * z.size), f"activation layer {so.dev_layer(m)}: {diff.size} of {z.size} inputs on the other side of zero"
            onet.force_act_side(li, side)
            kflips.append(int(diff.size))
    return pflips, kflips
