"""The evaluate()-mode input gradient (gr_net_backward_input_dev) and the noise refinement built on it, restated for the tests:

* the dispatch of the frozen pipeline backward (elem.hip launch_post_backward_frozen) and the input-only route's choice of data-gradient kernel
  (net.hip backward_input_impl: dgrad_conv3 / dgrad_convk / dgrad_group / dgrad_linear) as named features, with the timer labels of each;
* the case table of tests/test_gpu_refine.py and the inputs of every case;
* the float64 reference: a layer-descriptor list in PyTorch on the CPU, evaluate() mode (running statistics, Dropout as evaluate() has it),
  autograd for the gradient with respect to the input - with switches that degrade it on purpose (tests/test_refine_host.py shows the checks
  reject them);
* the refinement loop (per-row MSE, optim.adam on z, best-keeping) in float64 and in float32.
Nothing here touches the GPU."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import ganrev._lib as L
import g4_oracle                      # KINK_GAP: the conditioning rule its PReLU tests use
import torch_twin                     # the layer kinds both twins share

assert (torch_twin.CONV3, torch_twin.BN, torch_twin.LINEAR, torch_twin.CONVK, torch_twin.PRELU) == (L.CONV3, L.BN, L.LINEAR, L.CONVK, L.PRELU)

U = 2.0 ** -24
EPS = 1e-5
GRAD_RTOL = 1e-4                      # helpers.assert_grads_close's rtol: the project's bar on a gradient
KINK_GAP = g4_oracle.KINK_GAP         # no input of a ReLU / LeakyReLU / PReLU closer to zero than this
POOL_GAP = 1e-5                       # helpers.GAPS[0]: the two largest values of a max-pool window are this far apart (or equal)

# ---------------------------------------------------------------------------------------------------------------- the dispatch, restated
FROZEN_VEC, FROZEN_SCALAR = "post_backward_frozen_vec_kernel", "post_backward_frozen_kernel"
# data-gradient families -> the timer labels (prefixes) their launches carry
FAMILY_LABELS = {
    "conv3_split": ("conv3x3_split_kernel<", "conv3x3_split_wide_kernel<"),                # bf16x6 / f16x3 on the backward split image
    "conv3_f32": ("conv3x3_mfma_kernel<", "conv3x3_fewout_kernel<"),                       # fp32 MFMA (or the few-output VALU kernel) on wt_bwd
    "conv5_split": ("conv5x5_split_kernel<",),
    "convk_f32": ("convk_direct_kernel<", "convk_direct_sliced_kernel<", "convk_weight_image_kernel"),
    "conv1x1": ("conv1x1_kernel(dgrad)",),
    "linear": ("gemm_mfma_kernel", "gemm_f16x3_kernel", "gemm_f16x3_big_kernel", "gemm_splitk_reduce_kernel"),
    "grouplinear": ("grouplinear_dgrad_kernel",),
    "groupconv3_f32": ("groupconv3_dgrad_kernel",),
    "groupconv3_mfma": ("groupconv3_mfma_dgrad_kernel",),
    "prelu_multi": ("prelu_multi_backward_kernel",),
}
# what a full backward launches on top: none of it may appear under the input-only call
FORBIDDEN = ("wgrad", "prelu_grad_kernel", "prelu_multi_grad_kernel", "bias_grad", "post_backward_a", "post_backward_b", "post_backward_finalize",
             "bn_stats", "penalty_clamp")
GROUP_MFMA_MIN_TILES = 512            # groupmfma.hip's default of gr_set_tuning "group_mfma_min_tiles"
GM_PLANES, GM_MAX_HW = 16, 32         # groupconv3_mfma_supported: 16 planes per group, planes of at most 32 x 32

# one stage of a compiled net, as far as the input-only backward looks at it: kind in elem | conv3 | convk | linear | grouplin | groupconv | prelu_multi;
# C, H, W = the main operator's output (an element-wise stage: its input); pool None | "max" | "avg"; conv stages: Cin, up, fullconv, ksz; groups
St = collections.namedtuple("St", "kind C H W pool Cin up fullconv ksz groups", defaults=(None, 0, False, False, 3, 0))


def frozen_label(st, B):
    """launch_post_backward_frozen's shape rule (= launch_post_backward's): float4 when the rows split into float4s on both sides of the pool"""
    if st.kind == "prelu_multi":
        return None                   # nn.PReLU(n) is a stage of its own: launch_prelu_multi_backward alone
    vec = (st.W % 8 == 0 and st.H % 2 == 0) if st.pool else st.W % 4 == 0
    vec = vec and st.H * st.W >= 64 and float(B) * st.C * st.H * st.W < 4.0e9
    return FROZEN_VEC if vec else FROZEN_SCALAR


def dgrad_family(st, mode, B, group_mfma_min_tiles=GROUP_MFMA_MIN_TILES):
    """the data-gradient kernel family backward_input_impl picks for a stage (None: an element-wise stage has none); mode f32 | bf16x6 | f16x3"""
    m = ("f32", "bf16x6", "f16x3").index(mode)
    if st.kind == "elem":
        return None
    if st.kind == "prelu_multi":
        return "prelu_multi"
    if st.kind == "linear":
        return "linear"
    if st.kind == "grouplin":
        return "grouplinear"
    if st.kind == "groupconv":
        per = st.C // st.groups
        ok = per == GM_PLANES and st.Cin == st.C and st.H <= GM_MAX_HW and st.W <= GM_MAX_HW and (not st.up or (st.H % 2 == 0 and st.W % 2 == 0))
        return "groupconv3_mfma" if m != 0 and ok and B * st.groups >= group_mfma_min_tiles else "groupconv3_f32"
    if st.kind == "convk":
        if st.ksz == 1:
            return "conv1x1"
        split = lambda ci, co: ci >= 16 and ci % 8 == 0 and st.W >= 8 and st.H >= 4            # conv5x5_split_supported
        return "conv5_split" if m == 2 and st.ksz == 5 and split(st.Cin, st.C) and split(st.C, st.Cin) else "convk_f32"
    assert st.kind == "conv3"
    # dgrad3: plain stages take the split kernel in either split mode; up-sampling / full-conv stages only above 4 input planes
    return "conv3_split" if m >= 1 and ((not st.up and not st.fullconv) or st.Cin > 4) else "conv3_f32"


def expected_labels(stages, mode, B, group_mfma_min_tiles=GROUP_MFMA_MIN_TILES):
    """(exact labels that must appear, label prefixes that may appear) under one gr_net_backward_input_dev call"""
    must, may = set(), []
    for st in stages:
        fl = frozen_label(st, B)
        if fl:
            must.add(fl)
        fam = dgrad_family(st, mode, B, group_mfma_min_tiles)
        if fam:
            may.extend(FAMILY_LABELS[fam])
    return must, tuple(may)


def check_labels(ran, stages, mode, B, what, group_mfma_min_tiles=GROUP_MFMA_MIN_TILES):
    must, may = expected_labels(stages, mode, B, group_mfma_min_tiles)
    for k in ran:
        assert not any(f in k for f in FORBIDDEN), f"{what}: the input-only backward launched {k}"
        assert k in must or any(k.startswith(p) for p in may), f"{what} [{mode}]: launched {k}; the mirror expects {sorted(must)} and {may}"
    assert must <= set(ran), f"{what} [{mode}]: expected {sorted(must)}, ran {sorted(ran)}"
    fams = [f for f in (dgrad_family(st, mode, B, group_mfma_min_tiles) for st in stages) if f]
    for fam in fams:
        assert any(k.startswith(p) for k in ran for p in FAMILY_LABELS[fam]), f"{what} [{mode}]: no launch of the {fam} family among {sorted(ran)}"


def features(case, mode):
    """the named features a case reaches in one arithmetic mode"""
    out = set()
    for st in case.stages:
        out.add(frozen_label(st, case.B) or "prelu_multi")
        fam = dgrad_family(st, mode, case.B, case.tuning.get("group_mfma_min_tiles", GROUP_MFMA_MIN_TILES))
        if fam:
            out.add(fam)
    for d in case.descs:
        if d[0] in (L.ELU, L.RELU, L.LEAKYRELU, L.SIGMOID, L.TANH):
            out.add("act:" + {L.ELU: "ELU", L.RELU: "ReLU", L.LEAKYRELU: "LeakyReLU", L.SIGMOID: "Sigmoid", L.TANH: "Tanh"}[d[0]])
        if d[0] == L.PRELU and d[1] < 2:
            out.add("act:PReLU")
        if d[0] == L.BN:
            out.add("bn")
        if d[0] == L.MAXPOOL2:
            out.add("pool:max")
        if d[0] == L.AVGPOOL2:
            out.add("pool:avg")
        if d[0] == L.SPATIAL_DROPOUT:
            out.add("mask:scale")                 # evaluate(): x * (1 - p)
        if d[0] == L.DROPOUT:
            out.add("mask:elem" if d[5] & L.DROPOUT_ALWAYS_ON else ("mask:scale" if not d[5] & L.DROPOUT_V2 else "mask:none"))
    if not any(d[0] == L.BN for d in case.descs):
        out.add("no-bn")
    return out


ALL_FEATURES = frozenset({FROZEN_VEC, FROZEN_SCALAR, "prelu_multi", "bn", "no-bn", "pool:max", "pool:avg", "mask:scale", "mask:elem",
                          "act:ELU", "act:ReLU", "act:LeakyReLU", "act:Sigmoid", "act:Tanh", "act:PReLU"} | set(FAMILY_LABELS))
# reached only by shapes larger than a quick test should run (DESIGN.md says so): the 5x5 split data gradient needs >= 16 planes on both sides
NOT_IN_TABLE = frozenset({"conv5_split"})

# ---------------------------------------------------------------------------------------------------------------- the case table
_d = lambda kind, a=0, b=0, c=0, p=0.0, flags=0: (kind, a, b, c, float(p), flags)
conv, full, convk, lin = (lambda a, b: _d(L.CONV3, a, b)), (lambda a, b: _d(L.FULLCONV3, a, b)), (lambda a, b, k: _d(L.CONVK, a, b, k)), (lambda a, b: _d(L.LINEAR, a, b))
glin, gconv = (lambda a, b, g: _d(L.GROUPLINEAR, a, b, g)), (lambda a, b, g: _d(L.GROUPCONV3, a, b, g))
bn, prelu, view = (lambda c: _d(L.BN, c)), (lambda n=0: _d(L.PRELU, n)), (lambda a, b=1, c=1: _d(L.VIEW, a, b, c))
ELU_, RELU_, SIG_, TANH_, MAX_, AVG_, UP_ = _d(L.ELU), _d(L.RELU), _d(L.SIGMOID), _d(L.TANH), _d(L.MAXPOOL2), _d(L.AVGPOOL2), _d(L.UPSAMPLE2)
leaky = lambda s=0.2: _d(L.LEAKYRELU, p=s)
drop_v1 = lambda p=0.5: _d(L.DROPOUT, p=p)                                            # evaluate(): x * (1 - p)
drop_on = lambda p=0.5, v2=False: _d(L.DROPOUT, p=p, flags=L.DROPOUT_ALWAYS_ON | (L.DROPOUT_V2 if v2 else 0))      # the fixer's always-on Dropout
sdrop = lambda p=0.25: _d(L.SPATIAL_DROPOUT, p=p)

Case = collections.namedtuple("Case", "name group descs dims B stages tuning", defaults=({},))
ALL_MODES = ("f32", "bf16x6", "f16x3")

CASES = [
    # A: the frozen pipeline alone (element-wise nets; no convolution, so the arithmetic mode does not enter: f32)
    Case("A-bn-relu-3x5x7", "A", [bn(3), RELU_], (3, 5, 7), 3, [St("elem", 3, 5, 7)]),                                             # scalar path
    Case("A-bn-elu-max-8x8", "A", [bn(4), ELU_, MAX_], (4, 8, 8), 3, [St("elem", 4, 8, 8, "max")]),
    Case("A-prelu-sdrop-avg-8x16", "A", [prelu(), sdrop(), AVG_], (4, 8, 16), 3, [St("elem", 4, 8, 16), St("elem", 4, 8, 16, "avg")]),
    Case("A-bn-tanh-24", "A", [bn(24), TANH_], (24, 1, 1), 3, [St("elem", 24, 1, 1)]),                                             # what follows Linear 10 -> 24
    Case("A-bn-sigmoid-24", "A", [bn(24), SIG_], (24, 1, 1), 3, [St("elem", 24, 1, 1)]),
    Case("A-leaky-drop-8x8", "A", [leaky(), drop_v1()], (3, 8, 8), 3, [St("elem", 3, 8, 8)]),
    Case("A-always-on-drop-8x8", "A", [drop_on(), bn(3), ELU_], (3, 8, 8), 3, [St("elem", 3, 8, 8), St("elem", 3, 8, 8)]),
    Case("A-elu-max-drop-v2-on-8x8", "A", [ELU_, MAX_, drop_on(0.5, True)], (3, 8, 8), 3, [St("elem", 3, 8, 8, "max")]),           # mask 2 (behind the pool) from its bits
    Case("A-bn-elu-max-B1", "A", [bn(4), ELU_, MAX_], (4, 8, 8), 1, [St("elem", 4, 8, 8, "max")]),
    Case("A-bn-relu-odd-max-5x7", "A", [bn(3), RELU_, MAX_], (3, 5, 7), 3, [St("elem", 3, 5, 7, "max")]),                          # the pool drops the odd row / column
    # B: one-stage and two-stage nets
    Case("B-conv-sbn-elu-max", "B", [conv(4, 8), bn(8), ELU_, MAX_], (4, 8, 8), 3, [St("conv3", 8, 8, 8, "max", 4)]),
    Case("B-up-conv-8-4", "B", [UP_, conv(8, 4), bn(4), RELU_], (8, 4, 4), 3, [St("conv3", 4, 8, 8, None, 8, True)]),              # dgrad3: Cin > 4 -> split
    Case("B-up-conv-4-3", "B", [UP_, conv(4, 3), SIG_], (4, 4, 4), 3, [St("conv3", 3, 8, 8, None, 4, True)]),                      # dgrad3: Cin <= 4 -> fp32
    Case("B-conv5-6-5-9x6", "B", [convk(6, 5, 5), bn(5), leaky()], (6, 9, 6), 3, [St("convk", 5, 9, 6, None, 6, False, False, 5)]),
    Case("B-conv1x1", "B", [convk(6, 8, 1), bn(8), ELU_], (6, 8, 8), 3, [St("convk", 8, 8, 8, None, 6, False, False, 1)]),
    Case("B-fullconv-bn-leaky", "B", [full(6, 5), bn(5), leaky()], (6, 8, 8), 3, [St("conv3", 5, 8, 8, None, 6, False, True)]),
    Case("B-linear-bn-relu", "B", [lin(10, 24), bn(24), RELU_], (10, 1, 1), 3, [St("linear", 24, 1, 1, None, 10)]),
    Case("B-grouplinear", "B", [glin(12, 24, 4), bn(24), TANH_], (12, 1, 1), 3, [St("grouplin", 24, 1, 1, None, 12, False, False, 3, 4)]),
    Case("B-group-up-conv-default", "B", [UP_, gconv(64, 64, 4), bn(64), TANH_], (64, 8, 8), 3,
         [St("groupconv", 64, 16, 16, None, 64, True, False, 3, 4)]),          # (a smooth activation: 49 152 pre-activations cannot all keep KINK_GAP)
    Case("B-group-up-conv-mfma", "B", [UP_, gconv(64, 64, 4), bn(64), TANH_], (64, 8, 8), 3,
         [St("groupconv", 64, 16, 16, None, 64, True, False, 3, 4)], {"group_mfma_min_tiles": 1}),
    Case("B-prelu-multi", "B", [conv(4, 8), prelu(4), conv(8, 4), TANH_], (4, 8, 8), 3,
         [St("conv3", 8, 8, 8, None, 4), St("prelu_multi", 8, 8, 8), St("conv3", 4, 8, 8, None, 8)]),
    # C: no BatchNorm - the same data-gradient kernels as the training-mode backward, so the same bits
    Case("C-no-bn", "C", [conv(4, 8), prelu(), MAX_, conv(8, 8), leaky()], (4, 8, 8), 3,
         [St("conv3", 8, 8, 8, None, 4), St("elem", 8, 8, 8, "max"), St("conv3", 8, 4, 4, None, 8)]),
]
BY_NAME = {c.name: c for c in CASES}


def modes_of(case):
    return ("f32",) if case.group == "A" else ALL_MODES


# ---------------------------------------------------------------------------------------------------------------- inputs
def _layer_dims(descs, dims):
    """per layer, the per-sample dims of its INPUT"""
    out, (c, h, w) = [], dims
    for k, a, b, cc, _, _ in descs:
        out.append((c, h, w))
        if k in (L.CONV3, L.FULLCONV3, L.CONVK, L.GROUPCONV3):
            c = b
        elif k in (L.LINEAR, L.GROUPLINEAR):
            c, h, w = b, 1, 1
        elif k in (L.MAXPOOL2, L.AVGPOOL2):
            h, w = h // 2, w // 2
        elif k == L.UPSAMPLE2:
            h, w = h * 2, w * 2
        elif k == L.VIEW:
            c, h, w = a, max(b, 1), max(cc, 1)
    return out, (c, h, w)


def draw_params(descs, rng):
    """flat parameter vector in layer order (weight, bias | gamma, beta | slopes) and the running statistics of every BatchNorm, away from (0, 1)"""
    parts, running = [], []
    u = lambda n, lo, hi: rng.uniform(lo, hi, n).astype(np.float32)
    for k, a, b, c, _, _ in descs:
        if k in (L.CONV3, L.FULLCONV3, L.CONVK, L.GROUPCONV3, L.LINEAR, L.GROUPLINEAR):
            taps = 9 if k in (L.CONV3, L.FULLCONV3, L.GROUPCONV3) else (c * c if k == L.CONVK else 1)
            fan = (a // c if k in (L.GROUPCONV3, L.GROUPLINEAR) else a) * taps
            s = 1.0 / np.sqrt(fan)
            parts += [u(b * fan, -s, s), u(b, -0.05, 0.05)]
        elif k == L.BN:
            parts += [u(a, 0.5, 1.0), u(a, -0.2, 0.2)]
            running.append((u(a, -0.3, 0.3), u(a, 0.8, 1.5)))
        elif k == L.PRELU:
            parts.append(u(max(a, 1), 0.1, 0.4))
    return (np.concatenate(parts) if parts else np.zeros(0, np.float32)), running


def conditioned(rec):
    return rec["kink"] >= KINK_GAP and rec["pool_gap"] >= POOL_GAP


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Everything a case runs on, conditioned by seed (first seed whose float64 forward keeps every kink and pool near-tie away) -> dict; the arrays
    are shared between tests and read-only"""
    case = BY_NAME[name]
    lay, odims = _layer_dims(case.descs, case.dims)
    for seed in range(1, 60):
        rng = np.random.default_rng(7919 * seed + len(name))
        params, running = draw_params(case.descs, rng)
        masks = {}
        for i, (k, _, _, _, p, flags) in enumerate(case.descs):
            if k == L.DROPOUT and flags & L.DROPOUT_ALWAYS_ON:
                masks[i] = (rng.uniform(size=case.B * int(np.prod(lay[i]))) >= p).astype(np.uint8)
        shape = (case.B,) + (case.dims if case.dims[1:] != (1, 1) else case.dims[:1])
        x = rng.uniform(-1, 1, shape).astype(np.float32)
        oshape = (case.B,) + (odims if odims[1:] != (1, 1) else odims[:1])
        gout = rng.uniform(-1, 1, oshape).astype(np.float32)
        gout[np.abs(gout) < 0.05] = 0.5           # no tiny gradOutput: every dy element has digits to compare
        d = dict(params=params, running=running, masks=masks, x=x, gout=gout, seed=seed)
        ref = reference(case.descs, case.dims, d)
        if conditioned(ref):
            d["ref"] = ref
            for v in (params, x, gout, ref["gin"], ref["out"]):
                v.setflags(write=False)
            return d
    raise AssertionError(f"{name}: no seed keeps every kink {KINK_GAP:g} and every pool near-tie {POOL_GAP:g} away")


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def build(descs, dims, params, running, masks=None, dtype=torch.float64, degrade=None):
    """A layer-descriptor list in evaluate() mode as a PyTorch function x [B x ...] -> out [B x C x H x W]; rec (a dict) collects the conditioning
    of a pass.  degrade: None, or one of no_scale (the BatchNorm's gamma * invstd missing from the backward), batch_stats (batch statistics
    instead of the running ones), no_mask (a mask missing from the backward), no_pool_scatter (the max-pool gradient spread over the window)."""
    theta = torch.tensor(np.asarray(params, np.float64), dtype=dtype)
    masks = masks or {}
    off, P, bi = 0, [], 0
    for k, a, b, c, _, _ in descs:
        def take(n, shape):
            nonlocal off
            t = theta[off:off + n].reshape(shape)
            off += n
            return t
        if k in (L.CONV3, L.GROUPCONV3):
            g = c if k == L.GROUPCONV3 else 1
            P.append((take(b * (a // g) * 9, (b, a // g, 3, 3)), take(b, (b,))))
        elif k == L.FULLCONV3:
            P.append((take(a * b * 9, (a, b, 3, 3)), take(b, (b,))))
        elif k == L.CONVK:
            P.append((take(a * b * c * c, (b, a, c, c)), take(b, (b,))))
        elif k in (L.LINEAR, L.GROUPLINEAR):
            g = c if k == L.GROUPLINEAR else 1
            P.append((take(b * (a // g), (g, b // g, a // g)), take(b, (b,))))
        elif k == L.BN:
            rm, rv = running[bi]
            bi += 1
            P.append((take(a, (a,)), take(a, (a,)), torch.tensor(np.asarray(rm, np.float64), dtype=dtype), torch.tensor(np.asarray(rv, np.float64), dtype=dtype)))
        elif k == L.PRELU:
            P.append((take(max(a, 1), (max(a, 1),)),))
        else:
            P.append(None)
    assert off == theta.numel(), (off, theta.numel())
    ch = lambda t: t.reshape(1, -1, 1, 1)

    def through(value, grad_path):
        """`value` forward, the gradient of `grad_path` backward"""
        return grad_path + (value - grad_path).detach()

    def fwd(x, rec=None):
        rec = rec if rec is not None else {}
        rec.setdefault("kink", np.inf); rec.setdefault("pool_gap", np.inf); rec.setdefault("zmax", 0.0)
        B = x.shape[0]
        h = x.reshape((B,) + tuple(dims))
        for i, ((k, a, b, c, p, flags), q) in enumerate(zip(descs, P)):
            if k in (L.RELU, L.LEAKYRELU, L.PRELU):
                rec["kink"] = min(rec["kink"], float(h.detach().abs().min()))
            if k in (L.ELU, L.RELU, L.LEAKYRELU, L.PRELU, L.SIGMOID, L.TANH):
                rec["zmax"] = max(rec["zmax"], float(h.detach().abs().max()))
            if k in (L.CONV3, L.GROUPCONV3):
                h = F.conv2d(h, q[0], q[1], padding=1, groups=c if k == L.GROUPCONV3 else 1)
            elif k == L.FULLCONV3:
                h = F.conv_transpose2d(h, q[0], q[1], stride=1, padding=1)
            elif k == L.CONVK:
                h = F.conv2d(h, q[0], q[1], padding=c // 2)
            elif k in (L.LINEAR, L.GROUPLINEAR):
                g = q[0].shape[0]
                h = (torch.einsum("bgk,gmk->bgm", h.reshape(B, g, a // g), q[0]).reshape(B, b) + q[1]).reshape(B, b, 1, 1)
            elif k == L.BN:
                gamma, beta, rm, rv = q
                if degrade == "batch_stats":
                    z = F.batch_norm(h, None, None, gamma, beta, True, 0.1, EPS)
                else:
                    z = (h - ch(rm)) * ch(1.0 / torch.sqrt(rv + EPS)) * ch(gamma) + ch(beta)
                h = through(z, h) if degrade == "no_scale" else z
            elif k == L.ELU:
                h = F.elu(h)
            elif k == L.RELU:
                h = F.relu(h)
            elif k == L.LEAKYRELU:
                h = F.leaky_relu(h, float(np.float32(p)))
            elif k == L.PRELU:
                n = q[0].numel()
                h = torch.where(h > 0, h, ch(q[0].repeat_interleave(h.shape[1] // n)) * h)
            elif k == L.SIGMOID:
                h = torch.sigmoid(h)
            elif k == L.TANH:
                h = torch.tanh(h)
            elif k in (L.DROPOUT, L.SPATIAL_DROPOUT):
                p32 = float(np.float32(p))
                if k == L.DROPOUT and flags & L.DROPOUT_ALWAYS_ON:
                    keep = torch.tensor(masks[i].astype(np.float64), dtype=dtype).reshape(h.shape)
                    m = keep * (float(np.float32(1) / (np.float32(1) - np.float32(p))) if flags & L.DROPOUT_V2 else 1.0)
                elif k == L.SPATIAL_DROPOUT or not flags & L.DROPOUT_V2:
                    m = float(np.float32(1) - np.float32(p32))
                else:
                    m = 1.0
                h = through(h * m, h) if degrade == "no_mask" else h * m
            elif k == L.MAXPOOL2:
                hh = h[:, :, :h.shape[2] // 2 * 2, :h.shape[3] // 2 * 2].detach()
                win = hh.reshape(B, h.shape[1], h.shape[2] // 2, 2, h.shape[3] // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4).sort(dim=1).values
                gap = win[:, 3] - win[:, 2]
                gap = gap[gap > 0]
                if gap.numel():
                    rec["pool_gap"] = min(rec["pool_gap"], float(gap.min()))
                mp = F.max_pool2d(h, 2, 2)
                h = through(mp, F.avg_pool2d(h, 2, 2)) if degrade == "no_pool_scatter" else mp
            elif k == L.AVGPOOL2:
                h = F.avg_pool2d(h, 2, 2)
            elif k == L.UPSAMPLE2:
                h = h.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
            elif k == L.VIEW:
                h = h.reshape(B, a, max(b, 1), max(c, 1))
            else:
                raise ValueError(f"reference: kind {k}")
        return h
    return fwd


def reference(descs, dims, d, degrade=None):
    """out, gradInput (float64) of one (x, gradOutput) pair and the conditioning of the pass"""
    fwd = build(descs, dims, d["params"], d["running"], d["masks"], degrade=degrade)
    x = torch.tensor(np.asarray(d["x"], np.float64), requires_grad=True)
    rec = {}
    out = fwd(x, rec)
    out.backward(torch.tensor(np.asarray(d["gout"], np.float64)).reshape(out.shape))
    rec.update(out=out.detach().numpy().reshape(d["gout"].shape), gin=x.grad.numpy().copy())
    return rec


# ---------------------------------------------------------------------------------------------------------------- test A's constant
# Each dy element within c * 2^-24 * |dy_ref|.  The kernel's operations on one element, first order in u = 2^-24 (one rounding each):
#   g1 = gout * mask2 ; [avg: / 4, exact] ; g2 = g1 * mask1                                      2
#   dz = g2 * act'(z)  (a select for ReLU / LeakyReLU / PReLU / none: the product by the slope)   1 + rho_act
#   k = invstd * gamma, invstd itself rounded from double ; dy = dz * k                           3          (BatchNorm only)
# rho_act: the relative error of act'(z) as the kernel forms it from z = ((y - mean) * invstd) * gamma + beta.  z carries
#   dz_abs <= u (4 |z - beta| + |z|) <= u (5 Z + 4 BETA)       (sub, invstd's rounding, two products; the sum), Z = max|z|, BETA = max|beta|
# and with the project's constants for its activations on an fp32 argument (post_paths: ELU_ABS = 3e-7 = 5.04 u absolute on e^z, C_ACT Sigmoid 7,
# Tanh 4 relative on a):
#   ReLU / LeakyReLU / PReLU / none   0                                                     (the side of the kink is conditioned: KINK_GAP)
#   ELU      act' = (e^z - 1) + 1 for z <= 0:  (5.04 + 2) / e^-Z  +  dz_abs / u             (|d log act'/dz| = 1)
#   Sigmoid  act' = (1 - a) a:  7 + (7 e^Z + 1) + 1  +  dz_abs / u                          (1 - a carries a's error times a / (1 - a) = e^z; |d log act'/dz| <= 1)
#   Tanh     act' = 1 - a a:   (2 * 4 + 1) a^2 / (1 - a^2) + 1 / (1 - a^2)  +  2 dz_abs / u  at a = tanh Z      (|d log act'/dz| = 2 |a| <= 2)
# The inputs keep Z <= Z_MAX (asserted on the float64 pass) and |beta| <= 0.2.
Z_MAX, BETA_MAX = 1.7, 0.2


def c_bound(case):
    dz = 5.0 * Z_MAX + 4.0 * BETA_MAX if any(d[0] == L.BN for d in case.descs) else 0.0
    worst = 0.0
    for d in case.descs:
        if d[0] == L.ELU:
            worst = max(worst, 7.04 * np.exp(Z_MAX) + dz)
        elif d[0] == L.SIGMOID:
            worst = max(worst, 7.0 + 7.0 * np.exp(Z_MAX) + 1.0 + 1.0 + dz)
        elif d[0] == L.TANH:
            a2 = np.tanh(Z_MAX) ** 2
            worst = max(worst, (9.0 * a2 + 1.0) / (1.0 - a2) + 2.0 * dz)
    # an element-wise net of two stages (A-prelu-sdrop-avg, A-always-on-drop) runs the chain twice
    return len(case.stages) * (2.0 + 1.0 + 3.0) + worst


# ---------------------------------------------------------------------------------------------------------------- models
def model_spec(model, dims):
    """(descs, flat parameters in the compiled net's order, running statistics per BatchNorm layer of the net) of a ganrev.nn model, read from
    the host modules: no net is needed"""
    from ganrev import nn
    dims = tuple(int(v) for v in dims)
    descs = list(model._descs(dims)[0])
    flat = model._flat_host()
    perm = model._perm(dims)
    if perm is not None:
        flat = flat[np.asarray(perm)]
    bns = [m for m in model.leaves() if isinstance(m, nn.BatchNormalization)]
    groups = [[bns[i] for i in g] for g in model._plan(dims)[2]] if perm is not None else [[m] for m in bns]
    running = [(np.concatenate([m.running_mean for m in g]), np.concatenate([m.running_var for m in g])) for g in groups]
    return descs, flat, running


def shake_running(model, seed):
    """running statistics away from (0, 1), PReLU slopes apart: what a trained checkpoint carries"""
    rng = np.random.default_rng(seed)
    for m in model.leaves():
        if hasattr(m, "running_mean"):
            m.running_mean[...] = rng.uniform(-0.3, 0.3, m.running_mean.shape)
            m.running_var[...] = rng.uniform(0.6, 1.6, m.running_var.shape)
        if m.typename == "nn.PReLU":
            m.weight[...] = rng.uniform(0.1, 0.4)


# ---------------------------------------------------------------------------------------------------------------- the refinement loop
def adam_rows(z, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, eps_inside=False):
    """optim.adam as ganrev/optim.py specifies it (the step size formed in double and rounded to the tensors' precision once, epsilon outside the
    bias correction), on tensors of any precision, in place.  eps_inside: the degraded variant sqrt(v / bc2) + eps."""
    dt = z.dtype
    c = lambda s: torch.tensor(s, dtype=torch.float64).to(dt)
    m.mul_(c(beta1)).add_(c(1.0 - beta1) * g)
    v.mul_(c(beta2)).add_((c(1.0 - beta2) * g) * g)
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    if eps_inside:
        z.add_((c(-lr / bc1) * m) / (torch.sqrt(v / c(bc2)) + c(eps)))
    else:
        z.add_((c(-(lr * np.sqrt(bc2) / bc1)) * m) / (torch.sqrt(v) + c(eps)))


def refine_loop(fwd, images, z0, steps, lr, dtype=torch.float64, clamp=0.0, eps_inside=False, keep_best=True, chunk=None):
    """refine.refineNoise on the CPU: -> dict(z = best z per row, first, best = per-row losses, grads = the gradient of every step).  Rows are
    independent in evaluate() mode, so `chunk` changes nothing but the order of the work."""
    N = z0.shape[0]
    x = torch.tensor(np.asarray(images, np.float64), dtype=dtype).reshape(N, -1)
    z = torch.tensor(np.asarray(z0, np.float64), dtype=dtype)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    best, best_z, first, grads = torch.full((N,), np.inf, dtype=dtype), z.clone(), None, []
    for t in range(1, steps + 2):
        zz = z.clone().requires_grad_(True)
        loss = ((fwd(zz).reshape(N, -1) - x) ** 2).mean(dim=1)
        if t == 1:
            first = loss.detach().clone()
        better = loss.detach() < best if (keep_best or t == steps + 1) else torch.zeros(N, dtype=torch.bool)
        if not keep_best and t == steps + 1:
            better = torch.ones(N, dtype=torch.bool)                  # degraded: whatever the last step left
        best = torch.where(better, loss.detach(), best)
        best_z[better] = z[better]
        if t == steps + 1:
            break
        g, = torch.autograd.grad(loss.sum(), zz)
        grads.append(g.numpy().copy())
        adam_rows(z, g, m, v, t, lr, eps_inside=eps_inside)
        if clamp > 0:
            z.clamp_(-clamp, clamp)
    return dict(z=best_z.numpy(), first=first.numpy(), best=best.numpy(), grads=grads)


LOOP = dict(dims=(1, 16, 16), nd=8, rows=6, steps=5, lr=0.01)
NOISE_TOL = 1e-4                      # helpers.TOL: the project's bar on recovered noise vectors
G_COND = 1e-2                         # no Adam step decided by rounding: every |g| at least this share of the step's largest


def mini_g3(seed):
    from ganrev import models, synth
    G = models.create_G3(LOOP["dims"], LOOP["nd"], seed=seed)
    synth.init_params(G, seed)
    shake_running(G, seed + 100)
    return G


@functools.lru_cache(maxsize=None)
def loop_inputs():
    """The miniature G3 of tests D and F with targets x = G(z*) (float64, rounded to fp32) and a start z0 = z* + d, 0.2 <= |d_j| <= 0.4 (five Adam
    steps of 0.01 do not carry an entry across its optimum, where its gradient vanishes), the input seed chosen so that in the float64 loop no
    gradient entry of any step is below G_COND of that step's largest -> dict"""
    G = mini_g3(1)
    descs, flat, running = model_spec(G, (LOOP["nd"], 1, 1))
    fwd64 = build(descs, (LOOP["nd"], 1, 1), flat, running)
    for seed in range(1, 60):
        rng = np.random.default_rng(seed)
        zt = rng.standard_normal((LOOP["rows"], LOOP["nd"])).astype(np.float32)
        z0 = (zt + rng.uniform(0.2, 0.4, zt.shape) * rng.choice([-1.0, 1.0], zt.shape)).astype(np.float32)
        with torch.no_grad():
            images = fwd64(torch.tensor(zt.astype(np.float64))).numpy().astype(np.float32)
        r64 = refine_loop(fwd64, images, z0, LOOP["steps"], LOOP["lr"])
        cond = min(float(np.abs(g).min() / np.abs(g).max()) for g in r64["grads"])
        if cond >= G_COND:
            for a in (images, z0):
                a.setflags(write=False)
            return dict(seed=seed, model_seed=1, descs=descs, params=flat, running=running, images=images, z0=z0, r64=r64, cond=cond)
    raise AssertionError("no seed conditions the loop")
