"""What the device-resident training loops share (adversarial.DeviceGame, pretrain_g.DeviceLoop,
pretrain_with_previous_net.DeviceDistill): the executor that runs a ganrev.nn model on device tensors, the compile step in front of
it, an owner for the loops' device buffers and the periodic f16x3 range-guard scan.  Plain classes and functions a loop calls; no
base class to inherit from.  (Noise by method and the loss word are ctx.fill_noise / ctx.read_loss, ganrev._lib.)

The containers stay host code that enqueues work: every compiled part runs through gr_net_forward_dev / gr_net_backward_dev,
nn.Concat joins / slices / sums with gr_copy2d_dev / gr_add_dev, an nn.ConcatTable + nn.CAddTable pair (models.createResidual) sums its
branches with the same two calls, penalty + clamp + optim.adam are the fused gr_adam_step of each
part (gr_optim_step for the other five methods).  A model that compiles to one gr_net (G, R, the G autoencoder) is the trivial case: one forward_dev, one backward_dev.
"""
import numpy as np

from . import _lib as L
from . import nn

GUARD_PERIOD = 64       # batches between two f16x3 range-guard scans of the parameters (gr_range_guard_scan_params)


def compile_models(x, *models):
    """Compile every net of a chain of models with one small forward of the sample input x through them (parameters uploaded), WITHOUT
    side effects on the models: the reference has no such step, so the BatchNorm running statistics a training-mode forward writes
    on the device - and which evaluate()-mode users of G (train_r, apply_r) and the saved checkpoint would then carry - are put
    back from the host modules, which still hold the pre-compile values.  The forward stays: it is one tick of every net's Philox
    forward counter, which the dropout masks of all later batches depend on."""
    for m in models:
        x = m.forward(x)
    for m in models:
        m.push_bn_running()


def range_guard(ctx, batch, models):
    """In front of batch `batch` (1-based) of a loop whose *_dev calls are unguarded: every GUARD_PERIOD-th batch, the first included,
    an f16x3 context scans the parameters of every DeviceModel in `models`, as gr_train_r_step does."""
    if ctx.conv_mode() == "f16x3" and (batch - 1) % GUARD_PERIOD == 0:
        for m in models:
            m.range_guard_scan()


class Buffers:
    """Owner of device buffers: hands out what ctx.malloc returns and frees exactly what it handed out."""

    def __init__(self, ctx):
        self.ctx, self.nbytes, self.named = ctx, {}, {}      # pointer -> size of every live buffer; key -> pointer

    def malloc(self, nbytes):
        p = self.ctx.malloc(int(nbytes))
        self.nbytes[p] = int(nbytes)
        return p

    def adopt(self, p, nbytes):
        """take over a buffer somebody else got from ctx.malloc (a DeviceTensor handed over): freed like the others from now on"""
        self.nbytes[p] = int(nbytes)
        return p

    def floats(self, key, n):
        """the buffer kept under `key`, grown (never shrunk) to hold n floats"""
        p = self.named.get(key)
        if p is None or self.nbytes[p] < 4 * n:
            if p is not None:
                self.free(p)
            p = self.named[key] = self.malloc(4 * n)
        return p

    def free(self, p):
        del self.nbytes[p]
        self.ctx.free(p)

    def close(self):
        for p in list(self.nbytes):
            self.free(p)
        self.named.clear()


def _vol(d):
    return int(d[0]) * int(d[1]) * int(d[2])


class DeviceModel:
    """Device-resident executor of a compiled ganrev.nn model: one gr_net, or the parts of a model with an nn.Concat or with
    nn.ConcatTable + nn.CAddTable blocks.  It walks the containers themselves (nn's children(): a graph Sequential's parts(), a
    Concat's branches, a table block's branches), read once here because the tree is fixed once compiled and the walk runs four times
    a batch.

    A table block (models.lua:41-53): out = sum of the branch outputs, gradInput = sum of the branches' gradInputs, an nn.Identity
    branch contributing the block's input / gradOutput itself.  Both sums are formed in buffers of this executor, never in a branch's
    output: a training-mode stage output is state its net's backward reads."""

    def __init__(self, ctx, model):
        self.ctx, self.model, self.mem = ctx, model, Buffers(ctx)
        self.nets = [ch._net for ch, _, _ in model._param_chunks()]
        if any(n is None for n in self.nets):
            raise L.GanrevError("compile the model first (one forward)")
        if any(isinstance(m, nn.Concat) and m.dimension != 2 for m in model.listModules()):
            raise L.GanrevError("device-resident nn.Concat: only nn.Concat(2), the join along the feature / channel dimension "
                                "(models.lua:155,293)")
        self.kids, self.x = {}, {}          # id(container) -> its children() / the device input of its last forward (borrowed)
        self.branches = {}                  # id(table block) -> every branch, nn.Identity ones included
        todo = [model]
        for node in todo:
            self.kids[id(node)] = node.children()
            if isinstance(node, nn._TableSum):
                self.branches[id(node)] = node.modules[0].branches()
                if not self.kids[id(node)]:
                    raise L.GanrevError("device-resident nn.ConcatTable: at least one branch must hold a net")
            todo.extend(self.kids[id(node)] or ())
        for node in todo:
            # [B x C x H x W] branch outputs: joining channels in NCHW is joining each sample's features, which is what copy2d does -
            # as long as every branch has the same H x W (the host nn.Concat refuses the others at its first forward)
            if isinstance(node, nn.Concat) and len({self.out_dims(b)[1:] for b in self.kids[id(node)]}) > 1:
                raise L.GanrevError(f"device-resident nn.Concat(2): branch outputs {[self.out_dims(b) for b in self.kids[id(node)]]} do not line up")

    def out_dims(self, node):
        """per-sample (C, H, W) a node hands on"""
        kids = self.kids[id(node)]
        if kids is None:
            return tuple(int(d) for d in node._net.out_dims)
        if isinstance(node, nn.Concat):
            outs = [self.out_dims(b) for b in kids]
            return (sum(o[0] for o in outs),) + outs[0][1:]
        return self.out_dims(kids[-1])

    def out_features(self, node):
        kids = self.kids[id(node)]
        if kids is None:
            return _vol(node._net.out_dims)
        if isinstance(node, nn.Concat):
            return sum(self.out_features(b) for b in kids)
        return self.out_features(kids[-1])

    def in_features(self, node):
        kids = self.kids[id(node)]
        return _vol(node._net.in_dims) if kids is None else self.in_features(kids[0])

    def forward(self, x_dev, B, node=None):
        node = self.model if node is None else node
        self.x[id(node)] = x_dev
        kids = self.kids[id(node)]
        if kids is None:
            return node._net.forward_dev(x_dev, B)
        if isinstance(node, nn._TableSum):
            n = B * self.out_features(node)
            acc = self.mem.floats((id(node), "sum"), n)
            for j, b in enumerate(self.branches[id(node)]):
                o = x_dev if isinstance(b, nn.Identity) else self.forward(x_dev, B, b)
                if j == 0:
                    self.ctx.copy2d(acc, n // B, o, n // B, B, n // B)
                else:
                    self.ctx.add(acc, o, n)
            return acc
        if not isinstance(node, nn.Concat):
            for p in kids:
                x_dev = self.forward(x_dev, B, p)
            return x_dev
        total = self.out_features(node)
        cat = self.mem.floats((id(node), "cat"), B * total)
        lo = 0
        for b in kids:
            o, k = self.forward(x_dev, B, b), self.out_features(b)
            self.ctx.copy2d(cat + 4 * lo, total, o, k, B, k)
            lo += k
        return cat

    def backward(self, g_dev, B, want_gin, node=None, params=True):
        """gradOutput (device) -> gradInput (device pointer, or None when not wanted); accumulates every part's parameter gradient.
        params=False: nn.Module:updateGradInput in evaluate() mode - every part runs gr_net_backward_input_dev (after a forward with
        set_input_grad on), gradInput alone and no parameter gradient anywhere."""
        node = self.model if node is None else node
        x_dev = self.x[id(node)]
        kids = self.kids[id(node)]
        if not params and not want_gin:
            return None                   # nothing else is formed on this route
        if kids is None:
            gin = self.mem.floats((id(node), "gin"), B * _vol(node._net.in_dims)) if want_gin else None
            if params:
                node._net.backward_dev(x_dev, g_dev, B, gin)
            else:
                node._net.backward_input_dev(x_dev, g_dev, B, gin)
            return gin
        if isinstance(node, nn._TableSum):
            nin = B * self.in_features(node)
            acc = self.mem.floats((id(node), "gsum"), nin) if want_gin else None
            for j, b in enumerate(self.branches[id(node)]):
                gi = g_dev if isinstance(b, nn.Identity) else self.backward(g_dev, B, want_gin, b, params)
                if want_gin and j == 0:
                    self.ctx.copy2d(acc, nin // B, gi, nin // B, B, nin // B)
                elif want_gin:
                    self.ctx.add(acc, gi, nin)
            return acc
        if not isinstance(node, nn.Concat):
            for i in range(len(kids) - 1, -1, -1):
                g_dev = self.backward(g_dev, B, want_gin or i > 0, kids[i], params)
            return g_dev
        total, lo, acc = self.out_features(node), 0, None
        nin = B * self.in_features(node)
        for j, b in enumerate(kids):
            k = self.out_features(b)
            gs = self.mem.floats((id(node), "gslice", j), B * k)
            self.ctx.copy2d(gs, k, g_dev + 4 * lo, total, B, k)
            gi = self.backward(gs, B, want_gin, b, params)
            if want_gin:
                if acc is None:
                    acc = gi                      # the first branch's own gradInput buffer holds the sum
                else:
                    self.ctx.add(acc, gi, nin)
            lo += k
        return acc

    def zero_grads(self):
        for n in self.nets:
            n.zero_grads()

    def adam_step(self, hyper, t):
        for n in self.nets:
            n.adam_step(hyper, t)

    def adam_reset(self):
        for n in self.nets:
            n.adam_reset()

    def optim_step(self, config, t):
        for n in self.nets:
            n.optim_step(config, t)

    def optim_reset(self):
        for n in self.nets:
            n.optim_reset()

    def optim_state(self):
        """the two state vectors of every part joined in getParameters() order: (slot 0, slot 1) flat host arrays"""
        chunks = self.model._param_chunks()
        a, b = (np.zeros(max([hi for _, _, hi in chunks], default=0), np.float32) for _ in range(2))
        for ch, lo, hi in chunks:
            if hi > lo:
                a[lo:hi], b[lo:hi] = ch._net.optim_state()
        return a, b

    def set_training(self, training):
        for n in self.nets:
            n.set_training(training)

    def set_input_grad(self, on):
        for n in self.nets:
            n.set_input_grad(on)

    def range_guard_scan(self):
        for n in self.nets:
            n.range_guard_scan()

    def close(self):
        """Release the buffers of the executor (the nets stay with their model)."""
        self.mem.close()
        self.x.clear()
