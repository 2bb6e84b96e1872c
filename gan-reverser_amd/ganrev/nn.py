"""Host-side mirror of the Torch7 `nn` surface the reference scripts use, backed by libganrev.so.

Same names, argument meaning and error behaviour as the modules the reference instantiates
(reference models.lua:104-143, 389-464) and the protocol it calls on them:
  m:forward(input) -> m.output           train_r.lua:139,146 ; utils/nn_utils.lua:18
  m:backward(input, gradOutput)          train_r.lua:151
  m:training() / m:evaluate()            train_r.lua:70,189,222 ; apply_r.lua:64,94,103
  m:getParameters() -> flat, flatGrads   train_r.lua:122
  m:listModules(), m.modules[i]          utils/nn_utils.lua:395-426 ; weight-init.lua:52-72
Tensors are host numpy float32 arrays, contiguous NCHW — the reference's FloatTensors (train_r.lua:63);
the nn.Copy modules that bracket every reference model (models.lua:108,136,394,457) are accepted and ignored:
the host<->device crossing happens inside forward()/backward() exactly where those modules sat.

A Sequential is compiled into ONE gr_net on first use; leaf modules called on their own are one-layer nets.
"""
import math

import numpy as np

from . import _lib as L

# Torch7 draws every module's initial parameters from ONE process-wide generator (torch.manualSeed, train_r.lua:38-39), so two
# modules of equal shape never start out identical.  Constructors and reset() without an explicit rng draw from this one.
_RNG = np.random.default_rng(0)


def manualSeed(seed):
    """torch.manualSeed for parameter initialisation: restart the generator the constructors draw from."""
    global _RNG
    _RNG = np.random.default_rng(int(seed))


def _rng(rng=None):
    return rng if rng is not None else _RNG


class Module:
    __typename = "nn.Module"

    def __init__(self):
        self.train = True
        self.output = None
        self.gradInput = None
        self._net = None
        self._net_key = None
        self._flat = None          # (flatParams, flatGrads) after getParameters()
        self._pending_masks = {}
        self._ctx = None

    # ---- tree protocol
    @property
    def typename(self):
        return self.__class__.TYPENAME

    def listModules(self):
        return [self]

    def leaves(self):
        return [self]

    def desc(self, dims):
        """-> (list of (kind,a,b,c,p,flags), new dims).  dims = (C,H,W) per sample."""
        raise NotImplementedError

    def param_arrays(self):
        return []

    def set_param_arrays(self, arrays):
        pass

    def training(self):
        for m in self.listModules():
            m.train = True
        return self

    def evaluate(self):
        for m in self.listModules():
            if not getattr(m, "always_on", False):     # models.lua:404  drop.evaluate = function() end
                m.train = False
        return self

    def float(self):   # train_r.lua:78,104 — tensors are already float
        return self

    def cuda(self):    # models.lua:137,458 — device placement happens at compile time
        return self

    def zeroGradParameters(self):
        if self._flat is not None:
            self._flat[1][...] = 0
        if self._net is not None:
            self._net.zero_grads()

    def __repr__(self):
        return self.typename

    # ---- compilation
    def _context(self):
        if self._ctx is None:
            self._ctx = L.default_context()
        return self._ctx

    def _in_dims(self, x):
        if x.ndim == 4:
            return tuple(x.shape[1:])
        if x.ndim == 2:
            return (x.shape[1], 1, 1)
        raise ValueError(f"expected a batched 2-D or 4-D tensor, got shape {x.shape} "
                         "(BatchNormalization forces a batch dimension: apply_r.lua:330-331)")

    def _descs(self, dims):
        descs, index = [], {}
        d = dims
        for m in self.leaves():
            ds, d = m.desc(d)
            index[id(m)] = len(descs)
            descs.extend(ds)
        return descs, index

    def _compile(self, x):
        dims = self._in_dims(x)
        if self._net is not None and self._net_key == dims:
            return self._net
        if self._net is not None:
            self.pull_params()
            self._net.close()
        descs, self._layer_index = self._descs(dims)
        if not descs:
            raise L.GanrevError("empty module")
        self._net = L.Net(self._context(), descs, dims, perm=self._perm(dims))
        self._net_key = dims
        self.push_params()
        return self._net

    def _perm(self, dims):
        """net_flat = tree_flat[perm] when the compiled net orders its parameters differently from the tree (a bundle), else None"""
        return None

    def _bn_groups(self):
        """per BatchNorm layer of the compiled net, the BatchNorm modules whose running statistics it holds, concatenated in this order"""
        return [[m] for m in self.leaves() if isinstance(m, BatchNormalization)]

    def _flat_host(self):
        arrs = [a for m in self.leaves() for a in m.param_arrays()]
        if not arrs:
            return np.zeros(0, np.float32)
        return np.concatenate([a.ravel() for a in arrs]).astype(np.float32)

    def push_params(self):
        """host parameter arrays (+ BN running stats) -> device."""
        if self._net is None:
            return
        flat = self._flat[0] if self._flat is not None else self._flat_host()
        if flat.size:
            self._net.set_params(flat)
        self.push_bn_running()

    def push_bn_running(self):
        """host BatchNorm running statistics -> device (what a training-mode forward overwrote there: device.compile_models)"""
        for bi, mods in enumerate(self._bn_groups()):
            self._net.set_bn_running(bi, np.concatenate([m.running_mean for m in mods]), np.concatenate([m.running_var for m in mods]))

    def pull_params(self):
        """device -> host parameter arrays (+ BN running stats)."""
        if self._net is None:
            return
        flat = self._net.get_params()
        if self._flat is not None:
            self._flat[0][...] = flat
        else:
            off = 0
            for m in self.leaves():
                new = []
                for a in m.param_arrays():
                    new.append(flat[off:off + a.size].reshape(a.shape).copy())
                    off += a.size
                m.set_param_arrays(new)
        for bi, mods in enumerate(self._bn_groups()):
            mean, var = self._net.get_bn_running(bi)
            lo = 0
            for m in mods:
                m.running_mean, m.running_var = mean[lo:lo + m.nFeature].copy(), var[lo:lo + m.nFeature].copy()
                lo += m.nFeature

    def getParameters(self):
        """Flattens every parameter into one storage; module weight/bias become views into it (train_r.lua:122)."""
        if self._flat is None:
            n = self._param_count()
            self._bind_flat(np.zeros(n, np.float32), np.zeros(n, np.float32))
        return self._flat

    def _param_count(self):
        return int(sum(a.size for m in self.leaves() for a in m.param_arrays()))

    def _bind_flat(self, flat, grads):
        """Make `flat` / `grads` (given storage: a container hands each compiled part its slice) this module's flat vectors."""
        if self._net is not None:
            self.pull_params()
        flat[...] = self._flat_host()
        off = 0
        for m in self.leaves():
            views, gviews = [], []
            for a in m.param_arrays():
                views.append(flat[off:off + a.size].reshape(a.shape))
                gviews.append(grads[off:off + a.size].reshape(a.shape))
                off += a.size
            m.set_param_arrays(views)
            m.set_grad_arrays(gviews)
        self._flat = (flat, grads)

    def _param_chunks(self, lo=0):
        """[(module compiled into one gr_net, lo, hi)]: the slices of the flat vector each device net owns."""
        return [(self, lo, lo + self._param_count())]

    def set_grad_arrays(self, arrays):
        pass

    # ---- dropout noise injection (tests) / read-back
    def _leaf_layer(self, module):
        return self._layer_index[id(module)] + module.noise_layer_offset()

    def noise_layer_offset(self):
        return 0

    def setNoise(self, module, keep):
        """Use `keep` (0/1 per element of module's noise tensor) for the NEXT forward instead of Philox noise."""
        self._pending_masks[id(module)] = (module, np.ascontiguousarray(keep, dtype=np.uint8))

    def getNoise(self, module, batch):
        n = self._net.mask_size(self._leaf_layer(module), batch)
        return self._net.get_mask(self._leaf_layer(module), n)

    def manualSeed(self, seed):
        self._seed = int(seed)
        if self._net is not None:
            self._net.set_seed(self._seed)

    # ---- the nn.Module protocol
    def _prepare(self, x):
        """Everything :forward does before the data moves: compile for x's dims, seed, parameters, mode, injected noise."""
        net = self._compile(x)
        if getattr(self, "_seed", None) is not None and not getattr(self, "_seed_applied", False):
            net.set_seed(self._seed)
            self._seed_applied = True
        if self._flat is not None:
            net.set_params(self._flat[0])      # host storage is authoritative after getParameters()
        mods = [m for m in self.leaves() if not getattr(m, "always_on", False)] or self.leaves()
        net.set_training(any(m.train for m in mods))     # the fixer's always-on Dropout does not make the net "training"
        self._sync_modes(net)
        for module, keep in self._pending_masks.values():
            net.set_mask(self._leaf_layer(module), keep)
        self._pending_masks = {}
        return net

    def device_net(self, dims):
        """The compiled gr_net for per-sample input dims (C, H, W) / (n,), ready for the *_dev calls (no data moved): what the
        device-resident loops (apply_r.embed_dev, DeviceTrainer) drive instead of :forward."""
        dims = tuple(int(d) for d in (dims if len(dims) == 3 else (dims[0], 1, 1)))
        probe = np.empty((0,) + (dims if dims[1:] != (1, 1) else dims[:1]), np.float32)
        return self._prepare(probe)

    def forward(self, input):
        x = L.f32(input)
        net = self._prepare(x)
        b = x.shape[0]
        shape = (b,) + L.Net._shape(net.out_dims)
        if self.output is None or self.output.shape != shape:
            self.output = np.empty(shape, dtype=np.float32)
        net.forward(x, self.output)
        return self.output

    def _sync_modes(self, net):
        modes = {m.train for m in self.leaves() if not getattr(m, "always_on", False)}
        if len(modes) > 1:
            raise L.GanrevError("mixed training()/evaluate() modes inside one Sequential are not supported")

    updateOutput = forward

    def backward(self, input, gradOutput, scale=1):
        if scale != 1:
            raise L.GanrevError("only scale=1 is supported (nn.Sequential:backward default)")
        if self._net is None:
            raise L.GanrevError("backward called before forward")
        x, g = L.f32(input), L.f32(gradOutput)
        net = self._net
        if self._flat is not None:
            net.zero_grads()
        self.gradInput = net.backward(x, g, want_gin=True)
        if self._flat is not None:
            self._flat[1][...] += net.get_grads()  # accGradParameters accumulates into the flat gradient
        return self.gradInput

    def updateGradInput(self, input, gradOutput):
        """nn.Module:updateGradInput of a compiled model in evaluate(): gradInput alone - a frozen BatchNorm is an affine map, no parameter
        gradient is formed, no state moves.  The forward behind `input` is run again on the device with the parts' input-gradient flag on
        (the fused evaluate()-mode forward keeps no raw stage outputs) at the Philox counter of the forward it repeats, so an always-on
        Dropout draws the same noise; flag and counters are what they were when the call returns."""
        from . import device
        x, g = L.f32(input), L.f32(gradOutput)
        nets = [ch._net for ch, _, _ in self._param_chunks()]
        if not nets or any(n is None for n in nets):
            raise L.GanrevError("updateGradInput called before forward")
        if any(n.training for n in nets):
            raise L.GanrevError("updateGradInput is the evaluate()-mode input gradient; in training mode use backward")
        ctx, b = nets[0].ctx, x.shape[0]
        dm = device.DeviceModel(ctx, self)
        saved = [(n, n.forward_counter(), getattr(n, "input_grad", False)) for n in nets]
        xd = gd = None
        try:
            xd, gd = ctx.upload(x), ctx.upload(g)
            for n, counter, _ in saved:
                n.set_forward_counter(max(counter - 1, 0))
                n.set_input_grad(True)
            dm.forward(xd, b)
            self.gradInput = ctx.download(dm.backward(gd, b, True, params=False), x.shape)
        finally:
            for n, counter, flag in saved:
                n.set_input_grad(flag)
                n.set_forward_counter(counter)
            for p in (xd, gd):
                if p is not None:
                    ctx.free(p)
            dm.close()
        return self.gradInput


def _over_children(fn):
    """fn(self, children, ...) states what a container that runs as several compiled parts does with a call: it passes the call on
    to its children() and hands each its slice of the flat vector.  A plain Sequential has no children in this sense - it compiles
    to ONE gr_net - and answers as the Module it is."""
    base = getattr(Module, fn.__name__)

    def method(self, *args):
        kids = self.children()
        return base(self, *args) if kids is None else fn(self, kids, *args)
    method.__name__, method.__doc__ = fn.__name__, fn.__doc__ or base.__doc__
    return method


class _Container(Module):
    """What nn.Sequential and nn.Concat share: the list `modules` and the protocol over children()."""

    def __init__(self):
        super().__init__()
        self.modules = []

    def get(self, i):
        return self.modules[i - 1]     # Lua is 1-based

    def size(self):
        return len(self.modules)

    def listModules(self):
        return [self] + [x for m in self.modules for x in m.listModules()]

    def leaves(self):
        return [x for m in self.modules for x in m.leaves()]

    def children(self):
        """The containers this one runs as (each a Sequential or a Concat), or None when it compiles to one gr_net."""
        return None

    def _slices(self, kids, lo=0):
        """(child, lo, hi): each child's slice of this container's flat vector"""
        for p in kids:
            k = p._param_count()
            yield p, lo, lo + k
            lo += k

    @_over_children
    def _bind_flat(self, kids, flat, grads):
        for p, lo, hi in self._slices(kids):
            p._bind_flat(flat[lo:hi], grads[lo:hi])
        self._flat = (flat, grads)

    @_over_children
    def _param_chunks(self, kids, lo=0):
        return [c for p, plo, _ in self._slices(kids, lo) for c in p._param_chunks(plo)]

    @_over_children
    def push_params(self, kids):
        for p in kids:
            p.push_params()

    @_over_children
    def push_bn_running(self, kids):
        for p in kids:
            p.push_bn_running()

    @_over_children
    def pull_params(self, kids):
        for p in kids:
            p.pull_params()

    @_over_children
    def zeroGradParameters(self, kids):
        if self._flat is not None:
            self._flat[1][...] = 0
        for p in kids:
            p.zeroGradParameters()

    def _owner(self, module):
        """The compiled chunk a leaf module sits in (dropout-noise injection / read-back), or None"""
        kids = self.children()
        if kids is None:
            return self if any(m is module for m in self.leaves()) else None
        return next((o for o in (p._owner(module) for p in kids) if o is not None), None)

    def setNoise(self, module, keep):
        Module.setNoise(self._owner(module), module, keep)

    def getNoise(self, module, batch):
        return Module.getNoise(self._owner(module), module, batch)

    def __repr__(self):
        lines = [self._head() + " {"]
        lines += [f"  ({i + 1}): {m!r}" for i, m in enumerate(self.modules)]
        return "\n".join(lines + ["}"])


class Sequential(_Container):
    TYPENAME = "nn.Sequential"

    def add(self, m):
        self.modules.append(m)
        self._parts = None             # the execution plan of a model with an nn.Concat is rebuilt on the next use
        return self

    # ---- a Sequential that holds an nn.Concat (models.lua:293-321, the D network) cannot be one gr_net: it runs as a chain
    # of PARTS - every run of plain modules is compiled into one gr_net (a chunk), a branching container runs its branches.
    # Host arrays travel between the parts, as Torch7 tensors travel between the modules of the reference's containers.
    # An nn.ConcatTable followed by its nn.CAddTable (models.lua:41-53, createResidual) is ONE branching part: the table of branch
    # outputs exists only between the two.
    def _has_graph(self):
        return any(isinstance(m, (Concat, ConcatTable, CAddTable)) or (isinstance(m, Sequential) and m._has_graph()) for m in self.modules)

    def _is_graph(self):
        return self._has_graph() and self._bundle() is None

    def children(self):
        return self.parts() if self._is_graph() else None

    # ---- the bundle: an nn.Concat(2) of structurally identical branches (models.lua:155-172, create_G4) is one chain of grouped layers over
    # the concatenated features, so this Sequential compiles - with the modules behind the Concat - to ONE gr_net and is a plain net to every
    # caller (children() is None).  bundle_plan states the pattern and the translation.  `concat.bundle = False` before the first forward
    # keeps the parts route (tests, tools/bench_g4.py); not a user knob.
    def _bundle(self):
        """the nn.Concat this Sequential compiles as a bundle, or None"""
        cat = next((m for m in self.modules if isinstance(m, Concat)), None)
        key = None if cat is None else (id(cat), len(self.modules), len(cat.modules), sum(len(b.modules) for b in cat.modules), getattr(cat, "bundle", True))
        if getattr(self, "_bundle_key", ()) != key:
            self._bundle_key, self._bundle_plans = key, {}
            self._bundle_cat = cat if cat is not None and key[-1] and _bundle_pattern(self) is not None else None
        return self._bundle_cat

    def _plan(self, dims):
        dims = tuple(int(d) for d in dims)
        if dims not in self._bundle_plans:
            self._bundle_plans[dims] = bundle_plan(self, dims)
        return self._bundle_plans[dims]

    def _descs(self, dims):
        if self._bundle() is None:
            return Module._descs(self, dims)
        return list(self._plan(dims)[0]), {}          # (no layer index: a bundle holds no Dropout whose noise could be injected)

    def _perm(self, dims):
        return None if self._bundle() is None else self._plan(dims)[1]

    def _bn_groups(self):
        if self._bundle() is None:
            return Module._bn_groups(self)
        bns = [m for m in self.leaves() if isinstance(m, BatchNormalization)]
        return [[bns[i] for i in group] for group in self._plan(self._net_key)[2]]

    def parts(self):
        if getattr(self, "_parts", None) is None:
            parts, run = [], None
            mods = list(self.modules)
            while mods:
                m = mods.pop(0)
                if isinstance(m, CAddTable):
                    raise L.GanrevError("nn.CAddTable: only directly behind the nn.ConcatTable whose outputs it sums (models.lua:41-53)")
                if isinstance(m, ConcatTable):
                    if not mods or not isinstance(mods[0], CAddTable):
                        raise L.GanrevError("nn.ConcatTable: only with an nn.CAddTable directly behind it (models.lua:41-53)")
                    m = _TableSum(m, mods.pop(0))
                if isinstance(m, (Concat, _TableSum)) or (isinstance(m, Sequential) and m._has_graph()):
                    if run is not None:
                        parts.append(run)
                        run = None
                    parts.append(m)
                elif m.leaves():
                    if run is None:
                        run = Sequential()
                    run.add(m)
            if run is not None:
                parts.append(run)
            self._parts = parts
        return self._parts

    def forward(self, input):
        if not self._is_graph():
            return Module.forward(self, input)
        x = L.f32(input)
        self._part_inputs = []
        for p in self.parts():
            self._part_inputs.append(x)
            x = p.forward(x)
        self.output = x
        return x

    updateOutput = forward

    def backward(self, input, gradOutput, scale=1):
        if not self._is_graph():
            return Module.backward(self, input, gradOutput, scale)
        if getattr(self, "_part_inputs", None) is None:
            raise L.GanrevError("backward called before forward")
        g = L.f32(gradOutput)
        for p, x in zip(reversed(self.parts()), reversed(self._part_inputs)):
            g = p.backward(x, g, scale)
        self.gradInput = g
        return g

    def device_net(self, dims):
        if self._is_graph():
            raise L.GanrevError(f"this model runs as {len(self._param_chunks())} nets (it holds an nn.Concat or an nn.ConcatTable): the single-net "
                                "device-resident paths (forwardBatchedDev, apply_r.embed_dev, train_r's DeviceTrainer) cannot take it - use "
                                "the host-tensor paths (train_r --compat, apply_r --host) or device.DeviceModel")
        return Module.device_net(self, dims)

    def manualSeed(self, seed):
        if not self._is_graph():
            return Module.manualSeed(self, seed)
        for i, (chunk, _, _) in enumerate(self._param_chunks()):
            chunk.manualSeed(int(seed) * 1009 + i)

    def _head(self):
        return "nn.Sequential"


class Concat(_Container):
    """nn.Concat(dimension): every branch gets the same input, the outputs are joined along `dimension` (1-based, the batch
    is dimension 1): the D network's two convolution towers (models.lua:293-321, `nn.Concat(2)` of two [B x 512] feature
    vectors).  backward hands each branch its slice of gradOutput and sums the branches' gradInputs."""
    TYPENAME = "nn.Concat"

    def __init__(self, dimension):
        super().__init__()
        self.dimension = int(dimension)

    def add(self, m):
        if not isinstance(m, Sequential):
            m = Sequential().add(m)
        self.modules.append(m)
        return self

    def _is_graph(self):
        return True

    def children(self):
        return self.modules

    def forward(self, input):
        x = L.f32(input)
        outs = [b.forward(x) for b in self.modules]
        ax = self.dimension - 1
        if any(o.ndim <= ax or o.shape[:ax] != outs[0].shape[:ax] or o.shape[ax + 1:] != outs[0].shape[ax + 1:] for o in outs):
            raise L.GanrevError(f"nn.Concat({self.dimension}): branch outputs {[o.shape for o in outs]} do not line up")
        self._sizes = [o.shape[ax] for o in outs]
        self.output = np.concatenate(outs, axis=ax)
        return self.output

    updateOutput = forward

    def backward(self, input, gradOutput, scale=1):
        if getattr(self, "_sizes", None) is None:
            raise L.GanrevError("backward called before forward")
        x, g = L.f32(input), L.f32(gradOutput)
        ax, lo, gin = self.dimension - 1, 0, None
        for b, k in zip(self.modules, self._sizes):
            sl = [slice(None)] * g.ndim
            sl[ax] = slice(lo, lo + k)
            gi = b.backward(x, np.ascontiguousarray(g[tuple(sl)]), scale)
            gin = gi.copy() if gin is None else gin + gi
            lo += k
        self.gradInput = gin
        return gin

    def _head(self):
        return f"nn.Concat({self.dimension})"


class Identity(Module):
    """nn.Identity(): output = input, gradInput = gradOutput (createResidual's shortcut when the plane counts agree, models.lua:44).
    No layer of a gr_net: inside a plain Sequential it is skipped, as a ConcatTable branch it hands the input through."""
    TYPENAME = "nn.Identity"

    def leaves(self):
        return []

    def forward(self, input):
        self.output = input
        return input

    updateOutput = forward

    def backward(self, input, gradOutput, scale=1):
        self.gradInput = gradOutput
        return gradOutput


class ConcatTable(_Container):
    """nn.ConcatTable(): every branch gets the same input, the output is the list of branch outputs; backward sums the branches'
    gradInputs (models.lua:41-52).  `modules` holds what was added, as Torch7's does; a branch runs as a Sequential (its own, or
    one made around a single module), an nn.Identity as itself."""
    TYPENAME = "nn.ConcatTable"

    def __init__(self, *_ignored):       # models.lua:41 writes nn.ConcatTable(2); Torch7's constructor takes no argument
        super().__init__()
        self._runs = {}

    def add(self, m):
        self.modules.append(m)
        return self

    def branches(self):
        """what each entry of `modules` runs as: itself (a Sequential, an Identity) or a Sequential around it"""
        out = []
        for m in self.modules:
            if not isinstance(m, (Sequential, Identity)):
                if id(m) not in self._runs:
                    self._runs[id(m)] = Sequential().add(m)
                m = self._runs[id(m)]
            out.append(m)
        return out

    def _is_graph(self):
        return True

    def children(self):
        return [b for b in self.branches() if not isinstance(b, Identity)]      # the branches that compile to nets

    def forward(self, input):
        x = L.f32(input)
        self.output = [b.forward(x) for b in self.branches()]
        return self.output

    updateOutput = forward

    def backward(self, input, gradOutput, scale=1):
        x, gin = L.f32(input), None
        if len(gradOutput) != len(self.modules):
            raise L.GanrevError(f"nn.ConcatTable: {len(gradOutput)} gradOutputs for {len(self.modules)} branches")
        for b, g in zip(self.branches(), gradOutput):
            gi = b.backward(x, L.f32(g), scale)
            gin = gi.copy() if gin is None else gin + gi
        self.gradInput = gin
        return gin

    def _head(self):
        return "nn.ConcatTable"


class CAddTable(Module):
    """nn.CAddTable(inplace=false): the sum of a list of equally shaped tensors; the gradient goes unchanged to every entry
    (models.lua:53)."""
    TYPENAME = "nn.CAddTable"

    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = bool(inplace)

    def leaves(self):
        return []

    def forward(self, input):
        if not isinstance(input, (list, tuple)) or not input or any(np.shape(t) != np.shape(input[0]) for t in input):
            raise L.GanrevError("nn.CAddTable: expects a non-empty list of equally shaped tensors")
        out = np.array(input[0], dtype=np.float32, copy=True)
        for t in input[1:]:
            out += t
        self.output = out
        return out

    updateOutput = forward

    def backward(self, input, gradOutput, scale=1):
        self.gradInput = [gradOutput for _ in input]
        return self.gradInput


class _TableSum(_Container):
    """An nn.ConcatTable and the nn.CAddTable behind it as one part of a graph Sequential (Sequential.parts): out = sum of the branch
    outputs, gradInput = sum of the branches' gradInputs.  Not a module of the model's tree: listModules() / leaves() of the model
    never show it."""
    TYPENAME = "nn.Sequential"

    def __init__(self, table, add):
        super().__init__()
        self.modules = [table, add]

    def _is_graph(self):
        return True

    def children(self):
        return self.modules[0].children()

    def forward(self, input):
        table, add = self.modules
        self.output = add.forward(table.forward(input))
        return self.output

    updateOutput = forward

    def backward(self, input, gradOutput, scale=1):
        table, add = self.modules
        self.gradInput = table.backward(input, add.backward(table.output, L.f32(gradOutput), scale), scale)
        return self.gradInput

    def _head(self):
        return "nn.Sequential"


class Copy(Module):
    """nn.Copy(intype, outtype): host<->device crossing of the reference models — a no-op here."""
    TYPENAME = "nn.Copy"

    def __init__(self, intype=None, outtype=None, forceCopy=None, dontCast=None):
        super().__init__()

    def leaves(self):
        return []


class _Param(Module):
    def __init__(self):
        super().__init__()
        self.weight = self.bias = self.gradWeight = self.gradBias = None

    def param_arrays(self):
        return [self.weight, self.bias]

    def set_param_arrays(self, arrays):
        self.weight, self.bias = arrays

    def set_grad_arrays(self, arrays):
        self.gradWeight, self.gradBias = arrays


class SpatialConvolution(_Param):
    """nn.SpatialConvolution(nInputPlane, nOutputPlane, kW, kH, dW, dH, padW, padH) — 3x3 s1 p1 (the one geometry
    models.lua uses on the G/R path), 5x5 s1 p2 (the D network's createNxN(128, 64, 5, ..), models.lua:275,297) and 1x1 s1 p0
    (createResidual's pointwise layers, models.lua:25,36,47)."""
    TYPENAME = "nn.SpatialConvolution"
    KIND = L.CONV3

    def __init__(self, nInputPlane, nOutputPlane, kW=3, kH=3, dW=1, dH=1, padW=1, padH=None):
        super().__init__()
        padH = padW if padH is None else padH
        if (kW, kH, dW, dH, padW, padH) not in ((3, 3, 1, 1, 1, 1), (5, 5, 1, 1, 2, 2), (1, 1, 1, 1, 0, 0)) or (kW != 3 and self.KIND != L.CONV3):
            raise L.GanrevError("only 3x3 stride-1 pad-1 (models.lua:409-436), 5x5 stride-1 pad-2 (models.lua:297) and 1x1 stride-1 "
                                "pad-0 (models.lua:25) convolutions have a gfx950 kernel")
        self.nInputPlane, self.nOutputPlane, self.kW, self.kH = nInputPlane, nOutputPlane, kW, kH
        self.weight = np.zeros(self._wshape(), np.float32)
        self.bias = np.zeros(nOutputPlane, np.float32)
        self.reset()

    def _wshape(self):
        return (self.nOutputPlane, self.nInputPlane, self.kH, self.kW)

    def reset(self, stdv=None, rng=None):
        """nn.SpatialConvolution:reset — uniform(-stdv, stdv); a given stdv is scaled by sqrt(3) (upstream)."""
        rng = _rng(rng)
        stdv = stdv * math.sqrt(3) if stdv is not None else 1.0 / math.sqrt(self.kW * self.kH * self.nInputPlane)
        self.weight[...] = rng.uniform(-stdv, stdv, self.weight.shape)
        self.bias[...] = rng.uniform(-stdv, stdv, self.bias.shape)

    def desc(self, dims):
        c, h, w = dims
        if self.kW != 3:
            return [(L.CONVK, self.nInputPlane, self.nOutputPlane, self.kW, 0.0, 0)], (self.nOutputPlane, h, w)
        return [(self.KIND, self.nInputPlane, self.nOutputPlane, 0, 0.0, 0)], (self.nOutputPlane, h, w)

    def __repr__(self):
        p = (self.kW - 1) // 2
        return f"{self.typename}({self.nInputPlane} -> {self.nOutputPlane}, {self.kW}x{self.kH}, 1,1, {p},{p})"


class SpatialFullConvolution(SpatialConvolution):
    """nn.SpatialFullConvolution(nIn, nOut, 3,3,1,1,1,1): weight [nIn][nOut][3][3] (north_star names it; the
    reference itself up-samples with SpatialUpSamplingNearest + SpatialConvolution, models.lua:121-122)."""
    TYPENAME = "nn.SpatialFullConvolution"
    KIND = L.FULLCONV3

    def _wshape(self):
        return (self.nInputPlane, self.nOutputPlane, 3, 3)


class Linear(_Param):
    TYPENAME = "nn.Linear"

    def __init__(self, inputSize, outputSize):
        super().__init__()
        self.weight = np.zeros((outputSize, inputSize), np.float32)
        self.bias = np.zeros(outputSize, np.float32)
        self.reset()

    def reset(self, stdv=None, rng=None):
        rng = _rng(rng)
        stdv = stdv * math.sqrt(3) if stdv is not None else 1.0 / math.sqrt(self.weight.shape[1])
        self.weight[...] = rng.uniform(-stdv, stdv, self.weight.shape)
        self.bias[...] = rng.uniform(-stdv, stdv, self.bias.shape)

    def desc(self, dims):
        return [(L.LINEAR, self.weight.shape[1], self.weight.shape[0], 0, 0.0, 0)], (self.weight.shape[0], 1, 1)

    def __repr__(self):
        return f"nn.Linear({self.weight.shape[1]} -> {self.weight.shape[0]})"


class BatchNormalization(_Param):
    """nn.BatchNormalization(nFeature): eps 1e-5, momentum 0.1, affine (upstream defaults; the reference sets none)."""
    TYPENAME = "nn.BatchNormalization"

    def __init__(self, nFeature, eps=1e-5, momentum=0.1, affine=True):
        super().__init__()
        if eps != 1e-5 or momentum != 0.1 or not affine:
            raise L.GanrevError("only eps=1e-5, momentum=0.1, affine BatchNormalization is implemented")
        self.nFeature = nFeature
        self.weight = np.zeros(nFeature, np.float32)
        self.bias = np.zeros(nFeature, np.float32)
        self.running_mean = np.zeros(nFeature, np.float32)
        self.running_var = np.ones(nFeature, np.float32)
        self.reset()

    def reset(self, rng=None):
        rng = _rng(rng)
        self.weight[...] = rng.uniform(0, 1, self.weight.shape)   # upstream: weight:uniform(), bias:zero()
        self.bias[...] = 0
        self.running_mean[...] = 0
        self.running_var[...] = 1

    def desc(self, dims):
        return [(L.BN, self.nFeature, 0, 0, 0.0, 0)], dims

    def __repr__(self):
        return f"{self.typename}({self.nFeature})"


class SpatialBatchNormalization(BatchNormalization):
    TYPENAME = "nn.SpatialBatchNormalization"


class _Simple(Module):
    KIND = None

    def desc(self, dims):
        return [(self.KIND, 0, 0, 0, 0.0, 0)], dims


class ELU(_Simple):
    TYPENAME = "nn.ELU"
    KIND = L.ELU

    def __init__(self, alpha=1.0, inplace=False):
        super().__init__()
        if alpha != 1.0:
            raise L.GanrevError("nn.ELU: only alpha=1 (the reference's nn.ELU()) is implemented")


class ReLU(_Simple):
    TYPENAME = "nn.ReLU"
    KIND = L.RELU

    def __init__(self, inplace=False):
        super().__init__()


class Sigmoid(_Simple):
    TYPENAME = "nn.Sigmoid"
    KIND = L.SIGMOID


class Tanh(_Simple):
    TYPENAME = "nn.Tanh"
    KIND = L.TANH


class LeakyReLU(Module):
    TYPENAME = "nn.LeakyReLU"

    def __init__(self, negval=0.01, inplace=False):
        super().__init__()
        self.negval = float(negval)

    def desc(self, dims):
        return [(L.LEAKYRELU, 0, 0, 0, self.negval, 0)], dims


class PReLU(Module):
    """nn.PReLU(nOutputPlane=0): y = x > 0 ? x : w * x with ONE learnable slope w, initial value 0.25 (models.lua:276 and
    every other activation of the D networks).  The slope is a parameter: it sits in getParameters()' flat vector where
    the module sits in the network.  (The library's GR_PRELU also takes n >= 2 slopes - a bundle's PReLU layers, bundle_plan - but
    nn.PReLU(n) itself is still refused here: tests/test_host_logic.py pins the refusal.)"""
    TYPENAME = "nn.PReLU"

    def __init__(self, nOutputPlane=0):
        super().__init__()
        if nOutputPlane not in (0, None):
            raise L.GanrevError("nn.PReLU: only the shared slope (nn.PReLU() as models.lua writes it) is implemented")
        self.nOutputPlane = 0
        self.weight = np.full(1, 0.25, np.float32)
        self.gradWeight = None

    def param_arrays(self):
        return [self.weight]

    def set_param_arrays(self, arrays):
        (self.weight,) = arrays

    def set_grad_arrays(self, arrays):
        (self.gradWeight,) = arrays

    def desc(self, dims):
        return [(L.PRELU, 0, 0, 0, 0.0, 0)], dims


class Dropout(Module):
    """nn.Dropout(p=0.5, v1=false): v2 (default) scales kept units by 1/(1-p) while training and is the identity in
    evaluate(); v1 keeps the unscaled mask and multiplies by (1-p) in evaluate()."""
    TYPENAME = "nn.Dropout"

    def __init__(self, p=0.5, v1=False, inplace=False):
        super().__init__()
        self.p, self.v2, self.always_on = float(p), not v1, False

    def keepAlwaysOn(self):
        """models.lua:402-405:  drop:training(); drop.evaluate = function() end"""
        self.always_on = True
        self.train = True
        return self

    def desc(self, dims):
        flags = (L.DROPOUT_V2 if self.v2 else 0) | (L.DROPOUT_ALWAYS_ON if self.always_on else 0)
        return [(L.DROPOUT, 0, 0, 0, self.p, flags)], dims

    def __repr__(self):
        return f"nn.Dropout({self.p}{'' if self.v2 else ', v1'})"


class SpatialDropout(Module):
    TYPENAME = "nn.SpatialDropout"

    def __init__(self, p=0.5):
        super().__init__()
        self.p = float(p)

    def desc(self, dims):
        return [(L.SPATIAL_DROPOUT, 0, 0, 0, self.p, 0)], dims


class SpatialMaxPooling(Module):
    TYPENAME = "nn.SpatialMaxPooling"

    def __init__(self, kW, kH, dW=None, dH=None, padW=0, padH=0):
        super().__init__()
        dW, dH = dW or kW, dH or kH
        if (kW, kH, dW, dH, padW, padH) != (2, 2, 2, 2, 0, 0):
            raise L.GanrevError("only SpatialMaxPooling(2,2) is implemented (models.lua:422,440)")

    def desc(self, dims):
        c, h, w = dims
        return [(L.MAXPOOL2, 0, 0, 0, 0.0, 0)], (c, h // 2, w // 2)


class SpatialAveragePooling(Module):
    """nn.SpatialAveragePooling(kW, kH, dW, dH, padW, padH) (models.lua:71,235,242,249,348-363): only (2,2,2,2,0,0) has a
    kernel; Torch7's defaults (dW = dH = 1, ceil_mode false, count_include_pad true, divide true) are kept for the checkpoint"""
    TYPENAME = "nn.SpatialAveragePooling"

    def __init__(self, kW, kH, dW=1, dH=1, padW=0, padH=0):
        super().__init__()
        if (kW, kH, dW, dH, padW, padH) != (2, 2, 2, 2, 0, 0):
            raise L.GanrevError("only SpatialAveragePooling(2,2,2,2) is implemented (models.lua:71,235,242,249,348-363)")
        self.kW, self.kH, self.dW, self.dH, self.padW, self.padH = kW, kH, dW, dH, padW, padH

    def desc(self, dims):
        c, h, w = dims
        return [(L.AVGPOOL2, 0, 0, 0, 0.0, 0)], (c, h // 2, w // 2)


class SpatialUpSamplingNearest(Module):
    TYPENAME = "nn.SpatialUpSamplingNearest"

    def __init__(self, scale):
        super().__init__()
        if scale != 2:
            raise L.GanrevError("only SpatialUpSamplingNearest(2) is implemented (models.lua:121,127)")

    def desc(self, dims):
        c, h, w = dims
        return [(L.UPSAMPLE2, 0, 0, 0, 0.0, 0)], (c, h * 2, w * 2)


class View(Module):
    TYPENAME = "nn.View"

    def __init__(self, *sizes):
        super().__init__()
        self.sizes = tuple(int(s) for s in sizes)

    def desc(self, dims):
        s = self.sizes + (1,) * (3 - len(self.sizes))
        if int(np.prod(s)) != int(np.prod(dims)):
            raise L.GanrevError(f"nn.View{self.sizes}: input has {int(np.prod(dims))} elements per sample")
        return [(L.VIEW, s[0], s[1], s[2], 0.0, 0)], s


class Reshape(View):
    """nn.Reshape(size1, size2, ...) (models.lua:165, create_G4's branches): on a batched contiguous tensor what nn.View does - the
    same GR_VIEW layer - under its own class name, which the checkpoint keeps."""
    TYPENAME = "nn.Reshape"

    def desc(self, dims):
        s = self.sizes + (1,) * (3 - len(self.sizes))
        if int(np.prod(s)) != int(np.prod(dims)):
            raise L.GanrevError(f"nn.Reshape{self.sizes}: input has {int(np.prod(dims))} elements per sample")
        return [(L.VIEW, s[0], s[1], s[2], 0.0, 0)], s


# ---------------------------------------------------------------------------------------------------------------- the bundle
def _bundle_pattern(model):
    """The structural half of bundle_plan (no dims): -> (modules behind the Concat, the Concat) when `model` is a Sequential of [an
    nn.Concat(2) of >= 2 nn.Sequential branches with the same module types and sizes, module by module, the first an nn.Linear, every one
    of Linear | BatchNormalization | SpatialBatchNormalization | shared-slope PReLU | Reshape / View | SpatialUpSamplingNearest(2) | 3x3
    stride-1 pad-1 convolution] followed by plain modules only; else None."""
    if not isinstance(model, Sequential):
        return None
    mods = [m for m in model.modules if isinstance(m, _Container) or m.leaves()]          # (nn.Copy and nn.Identity are no layers)
    if not mods or not isinstance(mods[0], Concat) or any(isinstance(m, (_Container, CAddTable)) for m in mods[1:]):
        return None
    cat = mods[0]
    if cat.dimension != 2 or len(cat.modules) < 2:
        return None

    def sig(m):
        if type(m) is Linear:
            return ("linear",) + m.weight.shape
        if isinstance(m, BatchNormalization):
            return ("bn", m.nFeature)
        if type(m) is PReLU and m.nOutputPlane == 0:
            return ("prelu",)
        if isinstance(m, View):
            return ("view",) + m.sizes
        if isinstance(m, SpatialUpSamplingNearest):
            return ("up",)
        if isinstance(m, SpatialConvolution) and not isinstance(m, SpatialFullConvolution) and m.kW == 3:
            return ("conv", m.nInputPlane, m.nOutputPlane)
        return None
    sigs = []
    for b in cat.modules:
        if not isinstance(b, Sequential) or any(isinstance(m, _Container) for m in b.modules):
            return None
        sigs.append([sig(m) for m in b.modules if m.leaves()])
    first = sigs[0]
    if not first or None in first or first[0][0] != "linear" or any(s != first for s in sigs[1:]):
        return None
    return mods[1:], cat


def bundle_plan(model, dims):
    """-> (descs, perm, bn_map) when `model` compiles as a bundle (_bundle_pattern) for per-sample input dims, else None.  Pure: no GPU.
    With nb branches, per branch position:  first Linear(n, m) -> LINEAR(n, nb m);  later Linear(m, k) -> GROUPLINEAR(nb m, nb k, nb);
    BN(k) -> BN(nb k);  PReLU() -> PRELU(a = nb);  Reshape(c, h, w) -> VIEW(nb c, h, w);  up-sampling -> UPSAMPLE2;
    conv(c, c') -> GROUPCONV3(nb c, nb c', nb); then the modules behind the Concat as they are.
    perm: net_flat = tree_flat[perm] (the tree's getParameters() order is branch-major, the net's layer-major: per layer and parameter
    tensor, the branches' tensors one after another).  bn_map[i]: the indices, among the tree's BatchNorm modules in tree order, of the
    modules whose running statistics BatchNorm layer i of the net holds, concatenated."""
    pat = _bundle_pattern(model)
    if pat is None or getattr(pat[1], "bundle", True) is False:
        return None
    tail, cat = pat
    dims = tuple(int(d) for d in (dims if len(dims) == 3 else (dims[0], 1, 1)))
    nb = len(cat.modules)
    offs, bn_index, off = {}, {}, 0
    for m in model.leaves():
        offs[id(m)] = []
        for a in m.param_arrays():
            offs[id(m)].append((off, a.size))
            off += a.size
        if isinstance(m, BatchNormalization):
            bn_index[id(m)] = len(bn_index)
    descs, perm, bn_map = [], [], []

    def place(mods):
        """the parameter tensors of one layer: per tensor (weight, bias, ...), the modules' ranges one after another"""
        for q in range(len(offs[id(mods[0])])):
            for m in mods:
                lo, n = offs[id(m)][q]
                perm.append(np.arange(lo, lo + n, dtype=np.int64))
        if isinstance(mods[0], BatchNormalization):
            bn_map.append([bn_index[id(m)] for m in mods])
    branches = [[m for m in b.modules if m.leaves()] for b in cat.modules]
    d = dims
    for p, m in enumerate(branches[0]):
        (kind, a, b, c, pp, flags), = m.desc(d)[0]
        nd_ = m.desc(d)[1]
        if type(m) is Linear:
            descs.append((L.LINEAR, a, nb * b, 0, 0.0, 0) if p == 0 else (L.GROUPLINEAR, nb * a, nb * b, nb, 0.0, 0))
        elif isinstance(m, BatchNormalization):
            descs.append((L.BN, nb * a, 0, 0, 0.0, 0))
        elif type(m) is PReLU:
            descs.append((L.PRELU, nb, 0, 0, 0.0, 0))
        elif isinstance(m, View):
            descs.append((L.VIEW, nb * a, b, c, 0.0, 0))
        elif isinstance(m, SpatialUpSamplingNearest):
            descs.append((L.UPSAMPLE2, 0, 0, 0, 0.0, 0))
        else:
            descs.append((L.GROUPCONV3, nb * a, nb * b, nb, 0.0, 0))
        place([br[p] for br in branches])
        d = nd_
    d = (nb * d[0],) + tuple(d[1:])
    for m in tail:
        for x in m.leaves():
            ds, d = x.desc(d)
            descs.extend(ds)
            place([x])
    return descs, (np.concatenate(perm) if perm else np.zeros(0, np.int64)), bn_map


class MSECriterion:
    """nn.MSECriterion (sizeAverage): train_r.lua:119,147,150."""

    def __init__(self, sizeAverage=True):
        if not sizeAverage:
            raise L.GanrevError("only sizeAverage=true is implemented")
        self.output = 0.0
        self.gradInput = None

    def forward(self, input, target):
        self.output, self._g = L.default_context().mse(input, target)
        self._key = (id(input), id(target))
        return self.output

    def backward(self, input, target):
        _, g = L.default_context().mse(input, target)
        self.gradInput = g.reshape(np.shape(input))
        return self.gradInput


class BCECriterion:
    """nn.BCECriterion (sizeAverage): train.lua:173's CRITERION, used by adversarial.lua."""

    def __init__(self, sizeAverage=True):
        if not sizeAverage:
            raise L.GanrevError("only sizeAverage=true is implemented")
        self.output = 0.0
        self.gradInput = None

    def forward(self, input, target):
        self.output, _ = L.default_context().bce(input, target, want_grad=False)
        return self.output

    def backward(self, input, target):
        _, g = L.default_context().bce(input, target)
        self.gradInput = g.reshape(np.shape(input))
        return self.gradInput


class CosineDistance:
    """nn.CosineDistance on a pair of vectors (apply_r.lua:396-400)."""

    def forward(self, pair):
        a, b = pair
        self.output = np.array([L.default_context().cosine_similarity(a, b)], dtype=np.float32)
        return self.output
