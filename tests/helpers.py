"""Shared helpers for the parity tests: build a ganrev model and its oracle twin with identical parameters,
identical BN running stats and identical dropout noise."""
import numpy as np

from ganrev import synth

TOL = 1e-4   # north_star: recovered noise vectors and G images within 1e-4 fp32


def dropout_modules(model):
    return [m for m in model.leaves() if m.typename in ("nn.Dropout", "nn.SpatialDropout")]


def inject_noise(model, onet, B, seed, training=True):
    """Same keep flags into the HIP net (for its next forward) and the oracle net."""
    for m in dropout_modules(model):
        if not (training or getattr(m, "always_on", False)):
            continue
        li = onet.layer_index[id(m)]
        n = onet.mask_size(li, B)
        keep = synth.bernoulli_keep((n,), seed * 131 + li, m.p)
        onet.set_mask(li, keep)
        model.setNoise(m, keep)


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def assert_close(a, b, tol=TOL, what=""):
    d = maxdiff(a, b)
    assert np.isfinite(d) and d <= tol, f"{what}: max |diff| = {d:.3e} > {tol:g}"


def rel_close(a, b, rtol, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1e-30, float(np.max(np.abs(b))))
    d = float(np.max(np.abs(a - b))) / scale
    assert d <= rtol, f"{what}: max rel diff = {d:.3e} > {rtol:g}"


GAPS = (1e-5, 2e-6)     # tried in this order by the tests that search for a well-conditioned input


def pools_well_conditioned(model, onet, B, gap=2e-6):
    """True when no 2x2 max-pool window of the oracle's last forward has its two largest values closer than `gap`
    without being exactly equal.  A near-tie lets fp32 rounding pick a different argmax on the two sides, which re-routes
    a gradient: a legitimate difference that an element-wise tolerance cannot express.  The forward error of a correct fp32
    implementation at the pooling inputs is 2-3e-6 (all arithmetic modes), so two values closer than about 1e-5 can swap
    order; small cases can afford that gap (see pick_well_conditioned), a million-window tensor always holds a few such
    pairs and only the 2e-6 default is satisfiable there."""
    leaves = model.leaves()
    for i, m in enumerate(leaves):
        if m.typename != "nn.SpatialMaxPooling":
            continue
        li = onet.layer_index[id(leaves[i - 1])]
        x = onet.layer_output(li)
        pi = onet.layer_index[id(m)]
        n_out = onet.layer_output(pi).size
        # input is [B, C, H, W] with H*W = 4 * (out H*W)
        assert x.size // n_out == 4
        dims = onet.pool_in_dims[pi]
        xr = x.reshape(B, dims[0], dims[1] // 2, 2, dims[2] // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        srt = np.sort(xr, axis=1)
        g = srt[:, 3] - srt[:, 2]
        if np.any((g > 0) & (g < gap)):
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------
# Strict gradient parity around nn.SpatialMaxPooling.  A window whose two largest inputs differ by less than the forward
# error of a correct fp32 implementation (2-3e-6 here) may legitimately get a different argmax on the two sides; the gradient
# element it routes then lands elsewhere, which no element-wise tolerance can express.  Instead of budgeting for that, the
# tests (1) read the argmax both sides took (gr_net_get_pool_index / go_net_get_pool_index), (2) require the windows where
# they differ to be FEW and each to be a genuine near-tie in the oracle's own forward, and (3) re-run the oracle with the
# device's argmax forced, after which every gradient tensor is held to the strict bar.
NEAR_TIE = TOL       # (kink adoption of the small GAN cases only; the pool argmax uses near_tie_bar(mode) below)


def pool_layers(model, onet):
    """[(max-pool module, its layer index, per-sample input dims)] of a ganrev model / oracle twin pair."""
    return [(m, onet.layer_index[id(m)], onet.pool_in_dims[onet.layer_index[id(m)]])
            for m in model.leaves() if m.typename == "nn.SpatialMaxPooling"]


def current_mode():
    import ganrev._lib as L
    return L.default_context().conv_mode()


def _stage_before_pool(model, pool_module):
    """(conv, bn, elu) modules of the stage a nn.SpatialMaxPooling closes (models.lua:419-422, 436-440)."""
    leaves = model.leaves()
    i = leaves.index(pool_module)
    conv = bn = act = None
    for m in reversed(leaves[:i]):
        t = m.typename
        if t == "nn.ELU" and act is None: act = m
        elif t.endswith("BatchNormalization") and bn is None: bn = m
        elif t.endswith("SpatialConvolution"):
            conv = m
            break
    if conv is None or bn is None or act is None:
        return None            # not R's conv-SBN-ELU-[SpatialDropout]-MaxPool stage (the D network's BatchNorm-free PReLU stages)
    return conv, bn, act


def pool_input_error(model, onet, B, pool_module, y_dev, groups=1):
    """max |device - oracle| at the inputs of a max-pool, measured in THIS run: the device keeps the raw convolution output y of
    the stage (gr_net_layer_output of the conv layer) but never materialises BN -> ELU of it (fused into the pipeline kernel), so
    the device's pool input is rebuilt here from ITS y - batch-statistics BatchNorm (per data-parallel group) and ELU in float64 -
    and compared with the oracle's ELU output.  (A SpatialDropout between ELU and pool multiplies by 0 / 1: it cannot enlarge
    the error.)  The rebuild leaves out the device's own fp32 rounding of BN + ELU (~1e-7 relative)."""
    conv, bn, act = _stage_before_pool(model, pool_module)
    segs = {(id(m), nm): (lo, hi) for m, nm, lo, hi in param_segments(model)}
    gamma = onet.params[slice(*segs[(id(bn), "weight")])].astype(np.float64)
    beta = onet.params[slice(*segs[(id(bn), "bias")])].astype(np.float64)
    ref = onet.layer_output(onet.layer_index[id(act)])
    C = gamma.size
    y = np.asarray(y_dev).reshape(B, C, -1)
    ref = ref.reshape(B, C, -1)
    per, err = B // groups, 0.0
    for g in range(groups):
        yg = y[g * per:(g + 1) * per].astype(np.float64)
        mean = yg.mean(axis=(0, 2), keepdims=True)
        var = yg.var(axis=(0, 2), keepdims=True)
        z = (yg - mean) / np.sqrt(var + 1e-5) * gamma[None, :, None] + beta[None, :, None]
        z = np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
        err = max(err, float(np.abs(z - ref[g * per:(g + 1) * per]).max()))
    return err


# documented argmax flips per full-size step: windows that differ, summed over both pool layers;
# the full-size tests allow 4 x these
DOCUMENTED_FLIPS = {"cfg2": 5, "cfg3": 110}


def adopt_device_argmax(model, onet, B, max_flips, dev_index=None, dev_y=None, groups=1, mode=None, report=None):
    """Compare the pool argmax of the device's and the oracle's last forward, assert the differences are few genuine
    near-ties, force the device's argmax onto the oracle.
    The near-tie bar is DERIVED, per run, layer and arithmetic, from the forward error MEASURED at that pool's inputs
    (pool_input_error): the device takes j where the oracle takes i only if o_i - o_j <= e_j - e_i <= 2 max|e|, so a legitimate
    flip has a gap of at most twice the measured error (+1e-6 for the device's own fp32 rounding of BN + ELU, which the rebuild
    leaves out), capped by the 1e-4 forward tolerance the error itself is held to (measured on MI355X:
    errors 5e-6..2.7e-5 at the pool inputs - six convolutions deep, normalised by BatchNorm - and gaps up to 9.2e-6).
    dev_index / dev_y: {layer: array} when the device ran the batch in several pieces (data-parallel shards: per-shard arrays
    concatenated by the caller), else read from model._net.  Returns the number of differing windows per pool layer and prints
    them with the gaps (pytest -rP shows the line): a regression from "1-5 flips" to "30 flips" is visible in the log."""
    mode = mode or current_mode()
    flips, gaps, bars = [], [], []
    for m, li, (c, h, w) in pool_layers(model, onet):
        n = B * c * (h // 2) * (w // 2)
        dev = dev_index[li] if dev_index is not None else model._net.pool_index(li, n)
        ora = onet.pool_index(li)
        assert dev.size == n and dev.max() <= 3
        stage = _stage_before_pool(model, m)
        if stage is not None:
            cli = onet.layer_index[id(stage[0])]
            y = dev_y[cli] if dev_y is not None else model._net.layer_output(cli, (B * c * h * w,))
            ferr = pool_input_error(model, onet, B, m, y, groups)
            assert ferr <= TOL, f"pool layer {li} [{mode}]: forward error at the pool inputs {ferr:.3e} exceeds the forward bar {TOL:g}"
            bar = min(TOL, 2.0 * ferr + 1e-6)
        else:                  # the D network's small cases: no rebuildable pool input, the output tolerance is the bar
            ferr, bar = float("nan"), NEAR_TIE
        diff = np.nonzero(dev != ora)[0]
        gmax = 0.0
        if diff.size:
            x = onet.layer_output(li - 1).reshape(B * c, h // 2, 2, w // 2, 2).transpose(0, 1, 3, 2, 4).reshape(-1, 4)
            gap = x[diff, ora[diff]].astype(np.float64) - x[diff, dev[diff]].astype(np.float64)
            assert np.all(gap >= 0), "the oracle's argmax is not the maximum of its own window"
            gmax = float(gap.max())
            assert gmax < bar, (f"pool layer {li} [{mode}]: {diff.size} windows with a different argmax, largest gap {gmax:.3e} >= "
                                f"{bar:.2e} (2 x the forward error {ferr:.2e} measured at this pool's inputs): not a rounding-level near-tie")
        assert diff.size <= max_flips, f"pool layer {li} [{mode}]: {diff.size} of {n} windows differ in argmax (allowed {max_flips})"
        onet.force_pool_index(li, dev)
        flips.append(int(diff.size)); gaps.append(gmax); bars.append(bar)
    print(f"[argmax] mode={mode} B={B} flips per pool layer {flips}, largest gaps {['%.2e' % g for g in gaps]}, bars {['%.2e' % b for b in bars]}")
    if report is not None:
        report.update(flips=flips, gaps=gaps, bars=bars)
    return flips


def adopt_device_kinks(model, onet, B, max_flips):
    """The same for the kink of nn.ReLU / nn.LeakyReLU: an input within rounding noise of zero can land on either side, and the
    derivative jumps there by gout * (1 - slope) - one such element moves a BatchNorm bias gradient by more than the bar.
    The device never materialises the activation's input, but the sign of the stage output it does keep (after the Dropout
    that may follow; a dropped element passes no gradient on either side) tells the side it took.  Requires the elements
    where that differs from the oracle's own side to be few and within NEAR_TIE of zero in the oracle's forward, then forces
    the device's side onto the oracle's backward (go_net_force_act_side).  Returns the number of such elements per layer;
    activations whose stage output the device does not keep as fp32 (a max-pool follows, lean f16x3 stages) stay unforced."""
    import ganrev._lib as L
    leaves = model.leaves()
    flips = []
    for i, m in enumerate(leaves):
        if m.typename not in ("nn.ReLU", "cudnn.ReLU", "nn.LeakyReLU", "nn.PReLU"):      # cudnn.ReLU: G's activations (models.lua:117)
            continue
        li = onet.layer_index[id(m)]
        z = onet.layer_output(li - 1)
        own = z > 0
        lj = li + 1 if i + 1 < len(leaves) and leaves[i + 1].typename in ("nn.Dropout", "nn.SpatialDropout") else li
        if m.typename == "nn.PReLU":        # closes its stage on the device: its own output is kept (slope > 0: same sign as the input)
            lj = li
            assert float(m.weight[0]) > 0
        try:
            dev = model._net.layer_output(lj, (z.size,))
        except L.GanrevError:
            continue
        side = np.where(dev != 0, dev > 0, own if not m.typename.endswith(".ReLU") or lj != li else False)
        diff = np.nonzero(side != own)[0]
        if diff.size:
            assert np.abs(z[diff]).max() < NEAR_TIE, (f"activation layer {li}: {diff.size} inputs on the other side of zero, "
                                                      f"largest |input| {np.abs(z[diff]).max():.3e}: not rounding-level")
        assert diff.size <= max_flips, f"activation layer {li}: {diff.size} of {z.size} inputs on the other side of zero (allowed {max_flips})"
        onet.force_act_side(li, side)
        flips.append(int(diff.size))
    return flips


def release_argmax(model, onet):
    for m, li, _ in pool_layers(model, onet):
        onet.force_pool_index(li, None)


def param_segments(model):
    segs, off = [], 0
    for mod in model.leaves():
        for nm, arr in zip(("weight", "bias"), mod.param_arrays()):
            segs.append((mod, nm, off, off + arr.size)); off += arr.size
    return segs


def assert_grads_close(model, got, ref, rtol=1e-4, floor=1e-3, what=""):
    """Every parameter tensor's gradient within rtol of the largest reference gradient entry of ITS MODULE (weight and bias
    together).  Exception: a convolution / Linear bias directly in front of a BatchNorm has an exactly-zero true gradient
    (BatchNorm's backward makes sum(dy) vanish per channel): what both sides hold there is the rounding residue of a sum of
    B*H*W terms, not a quantity with digits to compare - it is required to BE residue on both sides (below 1e-3 of the
    module's weight gradient), which is what a wrong bias-gradient kernel would violate."""
    segs = param_segments(model)
    leaves = model.leaves()
    mod_max = {}
    for mod, nm, lo, hi in segs:
        mod_max[id(mod)] = max(mod_max.get(id(mod), 0.0), float(np.abs(ref[lo:hi]).max()))
    worst = 0.0
    for mod, nm, lo, hi in segs:
        r, g = ref[lo:hi], got[lo:hi]
        gmax = max(mod_max[id(mod)], floor)
        li = leaves.index(mod)
        before_bn = li + 1 < len(leaves) and leaves[li + 1].typename.endswith("BatchNormalization") and not mod.typename.endswith("BatchNormalization")
        if nm == "bias" and before_bn:
            assert float(np.abs(g).max()) <= 1e-3 * gmax and float(np.abs(r).max()) <= 1e-3 * gmax, \
                f"{what} {mod.typename}.bias [{lo}:{hi}] in front of BatchNorm: |g| {np.abs(g).max():.3e} (oracle {np.abs(r).max():.3e}) is not rounding residue of {gmax:.3e}"
            continue
        d = maxdiff(g, r)
        assert d <= rtol * gmax, f"{what} {mod.typename}.{nm} [{lo}:{hi}]: max |diff| {d:.3e} vs module max |g| {gmax:.3e}"
        # and per tensor in relative L2 (the max-norm bar alone is set by the module's largest entry)
        nr = float(np.linalg.norm(r.astype(np.float64)))
        if nr > floor * np.sqrt(r.size) * 1e-3:
            rel = float(np.linalg.norm(g.astype(np.float64) - r.astype(np.float64))) / nr
            worst = max(worst, rel)
            assert rel <= 3.0 * rtol, f"{what} {mod.typename}.{nm} [{lo}:{hi}]: relative L2 error {rel:.3e} > {3.0 * rtol:g}"
    print(f"[grads] {what} worst per-tensor relative L2 error {worst:.2e} (bar {3.0 * rtol:g})")


# ---------------------------------------------------------------------------------------------------------------------
# Oracle twin of a model that runs as several compiled parts (an nn.Concat inside: the D network, models.lua:272-337).  The
# oracle's go_net is a plain nn.Sequential, so the twin is one oracle net per compiled chunk of the ganrev model, chained on the
# host the way nn.Sequential / nn.Concat chain their children (the same composition rule the host mirror implements).
class OracleGraph:
    def __init__(self, oracle, model, in_dims):
        self.pairs = []          # (ganrev chunk, oracle net) in getParameters() order
        self.plan, self.out_dims = self._plan(oracle, model, tuple(in_dims))
        self.cache = {}

    def _plan(self, oracle, node, dims):
        from ganrev import nn
        if isinstance(node, nn.Concat):
            plans, outs = [], []
            for b in node.modules:
                pl, od = self._plan(oracle, b, dims)
                plans.append(pl); outs.append(od)
            ax = node.dimension - 2
            od = list(outs[0]); od[ax] = sum(o[ax] for o in outs)
            return ("concat", node.dimension - 1, plans), tuple(od)
        if node._is_graph():
            seq = []
            for p in node.parts():
                pl, dims = self._plan(oracle, p, dims)
                seq.append(pl)
            return ("seq", seq), dims
        onet = oracle.from_model(node, dims)
        self.pairs.append((node, onet))
        d = dims
        for m in node.leaves():
            _, d = m.desc(d)
        return ("net", onet), d

    def set_training(self, t):
        for _, o in self.pairs:
            o.set_training(t)

    def zero_grads(self):
        for _, o in self.pairs:
            o.zero_grads()

    @property
    def grads(self):
        return np.concatenate([o.grads for _, o in self.pairs])

    def forward(self, x):
        return self._fwd(self.plan, np.ascontiguousarray(x, np.float32))

    def _fwd(self, plan, x):
        self.cache[id(plan)] = x
        if plan[0] == "net":
            return np.array(plan[1].forward(x), copy=True)
        if plan[0] == "seq":
            for p in plan[1]:
                x = self._fwd(p, x)
            return x
        outs = [self._fwd(p, x) for p in plan[2]]
        self.cache[(id(plan), "sizes")] = [o.shape[plan[1]] for o in outs]
        return np.concatenate(outs, axis=plan[1])

    def backward(self, x, gout):
        return self._bwd(self.plan, np.ascontiguousarray(gout, np.float32))

    def _bwd(self, plan, g):
        x = self.cache[id(plan)]
        if plan[0] == "net":
            return np.array(plan[1].backward(x, g), copy=True)
        if plan[0] == "seq":
            for p in reversed(plan[1]):
                g = self._bwd(p, g)
            return g
        lo, gin = 0, None
        for p, k in zip(plan[2], self.cache[(id(plan), "sizes")]):
            sl = [slice(None)] * g.ndim
            sl[plan[1]] = slice(lo, lo + k)
            gi = self._bwd(p, np.ascontiguousarray(g[tuple(sl)]))
            gin = gi if gin is None else gin + gi
            lo += k
        return gin


# ------------------------------------------------------------------ sharded search, all ranks in one process
def tied_corpus(N, d, seed, needle, bounds):
    """A corpus whose exact-tie groups straddle shard boundaries (the merge order - score descending, GLOBAL row ascending - decides):
    * four bit-identical rows, one in each of the first four shards, nearly parallel to the needle row -> one tie group across THREE boundaries;
    * a duplicate of the needle row itself in the last shard (score ties with the needle's own hit);
    * a pair of identical rows in two middle shards.
    Returns (emb, rows of the 4-fold group)."""
    from ganrev import synth
    emb = synth.normal((N, d), seed)
    near = (emb[needle] + 0.05 * synth.normal((d,), seed + 1)).astype(np.float32)
    group = [lo + (hi - lo) // 3 for lo, hi in bounds[:4]]
    for r in group:
        emb[r] = near
    emb[bounds[-1][0] + 7] = emb[needle]
    emb[bounds[len(bounds) // 2][0] + 11] = emb[bounds[len(bounds) // 2 - 1][0] + 5]
    return emb, group


def sharded_search_in_process(local_topk, emb, bounds, needles, k):
    """ganrev.parallel.sharded_cosine_topk for every shard of `bounds`, one after the other in this process: each rank's candidate lists are caught at its
    all-gather and merged afterwards exactly as the ranks would (merge_candidates).  The needle exchange (sum all-reduce) returns what the sum over the
    ranks is: the needle rows."""
    from ganrev.parallel import merge_candidates, sharded_cosine_topk
    vec = emb[list(needles)].copy()

    class Comm:
        def __init__(self, r): self.rank, self.world, self.got = r, len(bounds), []
        def allreduce_sum(self, arr): return vec.copy()
        def allgather(self, arr):
            self.got.append(arr); return [arr]
    ci, cs = [], []
    for r, (lo, hi) in enumerate(bounds):
        c = Comm(r)
        sharded_cosine_topk(local_topk, emb[lo:hi], lo, needles, k, c)
        ci.append(c.got[0]); cs.append(c.got[1])
    return merge_candidates(ci, cs, k)


# ------------------------------------------------------------------ search reference, needles in parallel
def oracle_topk_parallel(oracle, emb, needles, k, accumulate_in_float=False, workers=None):
    """oracle.cosine_topk over slices of the needle list on a pool of threads, each running the oracle on one core (the oracle is a ctypes library:
    its calls release the GIL).  Every needle's answer is computed on its own (oracle_net.c: one full sort per needle), so the slicing changes no
    bit of the result.  The OpenMP thread count is per calling thread, so each worker sets its own."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    needles = np.ascontiguousarray(needles, dtype=np.int64)
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    workers = max(1, min(16, os.cpu_count() or 1, needles.size) if workers is None else workers)
    parts = [p for p in np.array_split(needles, workers) if p.size]
    oracle.lib()                    # (loaded once, here: the loader is not meant for several threads at once)

    def run(part):
        oracle.set_threads(1)
        return oracle.cosine_topk(emb, part, k, accumulate_in_float=accumulate_in_float)
    with ThreadPoolExecutor(max_workers=len(parts)) as ex:
        res = list(ex.map(run, parts))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
