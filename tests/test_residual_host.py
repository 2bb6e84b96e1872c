"""CPU: models.createResidual (reference models.lua:8-55) as a module tree - structure, repr, parameters, the Torch7 checkpoint
round trip - and the geometry nn.SpatialConvolution accepts.  Nothing here touches the GPU: modules are built, never run."""
import numpy as np
import pytest

import ganrev._lib as L
from ganrev import models, nn, t7, weight_init


def _types(seq):
    return [m.typename for m in seq.modules]


def _conv(m):
    return (m.nInputPlane, m.nOutputPlane, m.kW, m.kH)


def _triple(act_name, bn):
    return ["cudnn.SpatialConvolution"] + (["nn.SpatialBatchNormalization"] if bn else []) + [act_name]


# (in, inner, out): in = inner = out | in != inner = out | in = inner != out | all different
STRUCTURES = [(16, 16, 16), (16, 8, 8), (8, 8, 16), (6, 12, 10)]


@pytest.mark.parametrize("bn", [True, False])
@pytest.mark.parametrize("a,inner,c", STRUCTURES)
def test_module_tree(a, inner, c, bn):
    m = models.createResidual(a, inner, c, bn=bn)
    assert _types(m) == ["nn.ConcatTable", "nn.CAddTable"]
    table = m.modules[0]
    assert len(table.modules) == 2 and table.modules[0].typename == "nn.Sequential"
    body = table.modules[0]
    want = []
    if a != inner:
        want.append((a, inner, 1, 1))
    want += [(inner, inner, 3, 3), (inner, inner, 3, 3)]
    if inner != c:
        want.append((inner, c, 1, 1))
    assert _types(body) == _triple("cudnn.ReLU", bn) * len(want)
    assert [_conv(x) for x in body.modules if x.typename == "cudnn.SpatialConvolution"] == want
    if bn:
        assert [x.nFeature for x in body.modules if x.typename == "nn.SpatialBatchNormalization"] == [w[1] for w in want]
    short = table.modules[1]
    if a == c:
        assert short.typename == "nn.Identity"
    else:
        assert _types(short) == _triple("cudnn.ReLU", bn)
        assert _conv(short.modules[0]) == (a, c, 1, 1)
    # getParameters(): depth-first module order - the inner branch, then the shortcut; a convolution is weight then bias, BatchNorm
    # gamma then beta
    def block(i, o, k):
        return i * o * k * k + o + (2 * o if bn else 0)
    n_inner = sum(block(i, o, k) for i, o, k, _ in want)
    n_short = 0 if a == c else block(a, c, 1)
    flat, grads = m.getParameters()
    assert flat.size == grads.size == n_inner + n_short
    chunks = m._param_chunks()
    assert [(lo, hi) for _, lo, hi in chunks] == ([(0, n_inner)] if a == c else [(0, n_inner), (n_inner, n_inner + n_short)])
    first = body.modules[0]
    assert np.shares_memory(first.weight, flat) and np.array_equal(flat[:first.weight.size], first.weight.ravel())
    assert np.array_equal(flat[first.weight.size:first.weight.size + first.bias.size], first.bias)
    if a != c:
        sw = short.modules[0].weight
        assert np.array_equal(flat[n_inner:n_inner + sw.size], sw.ravel())
    assert [x.typename for x in m.listModules()][:3] == ["nn.Sequential", "nn.ConcatTable", "nn.Sequential"]
    assert [type(p).__name__ for p in m.parts()] == ["_TableSum"] and m._is_graph()


def test_repr():
    m = models.createResidual(4, 2, 4, "LeakyReLU")
    assert repr(m) == "\n".join([
        "nn.Sequential {",
        "  (1): nn.ConcatTable {",
        "  (1): nn.Sequential {",
        "  (1): cudnn.SpatialConvolution(4 -> 2, 1x1, 1,1, 0,0)",
        "  (2): nn.SpatialBatchNormalization(2)",
        "  (3): nn.LeakyReLU",
        "  (4): cudnn.SpatialConvolution(2 -> 2, 3x3, 1,1, 1,1)",
        "  (5): nn.SpatialBatchNormalization(2)",
        "  (6): nn.LeakyReLU",
        "  (7): cudnn.SpatialConvolution(2 -> 2, 3x3, 1,1, 1,1)",
        "  (8): nn.SpatialBatchNormalization(2)",
        "  (9): nn.LeakyReLU",
        "  (10): cudnn.SpatialConvolution(2 -> 4, 1x1, 1,1, 0,0)",
        "  (11): nn.SpatialBatchNormalization(4)",
        "  (12): nn.LeakyReLU",
        "}",
        "  (2): nn.Identity",
        "}",
        "  (2): nn.CAddTable",
        "}"])


def test_activations():
    relu = models.createResidual(4, 4, 4)
    assert relu.modules[0].modules[0].modules[2].typename == "cudnn.ReLU"
    assert _types(models.createResidual(4, 4, 4, "ReLU").modules[0].modules[0]) == _types(relu.modules[0].modules[0])
    pre = models.createResidual(4, 2, 6, "PReLU")
    slopes = [x for x in pre.leaves() if x.typename == "nn.PReLU"]
    assert len(slopes) == 5 and len({id(s.weight) for s in slopes}) == 5 and all(s.weight[0] == np.float32(0.25) for s in slopes)
    flat, _ = pre.getParameters()
    # one slope per activation, each where its module sits: 1x1 (4*2+2), BN (4), slope, ...
    assert flat[4 * 2 + 2 + 4] == np.float32(0.25) and flat.size == (8 + 2 + 4 + 1) + 2 * (36 + 2 + 4 + 1) + (12 + 6 + 12 + 1) + (24 + 6 + 12 + 1)
    leaky = [x for x in models.createResidual(4, 4, 4, "LeakyReLU").leaves() if x.typename == "nn.LeakyReLU"]
    assert len(leaky) == 2 and all(x.negval == 0.333 for x in leaky)
    with pytest.raises(ValueError, match="Unknown activation 'ELU'"):
        models.createResidual(4, 4, 4, "ELU")


def test_pointwise_geometry_and_init():
    nn.manualSeed(5)
    m = nn.SpatialConvolution(9, 4, 1, 1, 1, 1, 0, 0)
    assert m.weight.shape == (4, 9, 1, 1) and m.desc((9, 6, 6)) == ([(L.CONVK, 9, 4, 1, 0.0, 0)], (4, 6, 6))
    bound = 1.0 / np.sqrt(1 * 1 * 9)             # Torch7: stdv = 1 / sqrt(kW * kH * nInputPlane)
    assert np.abs(m.weight).max() <= bound and np.abs(m.weight).max() > 0.8 * bound and np.abs(m.bias).max() <= bound
    # weight-init.lua on a 1x1 window: fan_in = nInputPlane * 1 * 1, fan_out = nOutputPlane * 1 * 1
    seq = nn.Sequential().add(nn.SpatialConvolution(9, 4, 1, 1, 1, 1, 0, 0))
    weight_init.w_init(seq, "xavier")
    lim = np.sqrt(2.0 / (9 + 4)) * np.sqrt(3)
    w = seq.modules[0].weight
    assert np.abs(w).max() <= lim and np.abs(w).max() > 0.8 * lim and not seq.modules[0].bias.any()
    with pytest.raises(L.GanrevError):
        nn.SpatialConvolution(4, 4, 1, 1, 1, 1, 1, 1)         # a padding that does not match the window
    with pytest.raises(L.GanrevError):
        nn.SpatialConvolution(4, 4, 3, 3, 1, 1, 0, 0)
    with pytest.raises(L.GanrevError):
        nn.SpatialFullConvolution(4, 4, 1, 1, 1, 1, 0, 0)


def test_table_modules_on_host_arrays():
    """ConcatTable / CAddTable / Identity themselves (no net involved: Identity branches only)"""
    x = np.arange(6, dtype=np.float32).reshape(2, 3)
    table = nn.ConcatTable().add(nn.Identity()).add(nn.Identity())
    outs = table.forward(x)
    assert isinstance(outs, list) and len(outs) == 2 and all(np.array_equal(o, x) for o in outs)
    add = nn.CAddTable()
    assert np.array_equal(add.forward(outs), 2 * x) and np.array_equal(x, np.arange(6, dtype=np.float32).reshape(2, 3))
    g = np.ones_like(x)
    gs = add.backward(outs, g)
    assert len(gs) == 2 and all(t is g for t in gs)
    assert np.array_equal(table.backward(x, gs), 2 * g)
    with pytest.raises(L.GanrevError):
        nn.Sequential().add(nn.ConcatTable().add(nn.Identity())).parts()       # no CAddTable behind it
    with pytest.raises(L.GanrevError):
        nn.Sequential().add(nn.CAddTable()).parts()


def _signature(m):
    """the tree as (class, geometry, parameters): cudnn.* classes are written as their nn.* counterparts (t7.from_model)"""
    name = m.typename.replace("cudnn.", "nn.")
    if hasattr(m, "modules"):
        return (name, [_signature(x) for x in m.modules])
    extra = {k: getattr(m, k) for k in ("nInputPlane", "nOutputPlane", "kW", "kH", "nFeature", "negval", "inplace") if hasattr(m, k)}
    return (name, extra, [a.tobytes() for a in m.param_arrays()] + [getattr(m, k).tobytes() for k in ("running_mean", "running_var") if hasattr(m, k)])


@pytest.mark.parametrize("args", [(16, 16, 16, "ReLU"), (16, 8, 24, "PReLU"), (6, 12, 10, "LeakyReLU", False)])
def test_t7_round_trip(args):
    nn.manualSeed(7)
    m = models.createResidual(*args)
    for x in m.leaves():
        if hasattr(x, "running_mean"):
            x.running_mean[...] = np.linspace(-1, 1, x.nFeature); x.running_var[...] = np.linspace(0.5, 2, x.nFeature)
    data = t7.dumps(t7.from_model(m))
    back = t7.to_model(t7.load(data))
    assert _signature(back) == _signature(m)
    assert np.array_equal(back._flat_host(), m._flat_host()) and back._flat_host().size > 0
    assert t7.dumps(t7.from_model(back)) == data
    raw = t7.load(data)
    table, add = raw.fields["modules"]
    assert table.typename == "nn.ConcatTable" and add.typename == "nn.CAddTable" and add.fields["inplace"] is False
    convs = [x for x in table.fields["modules"][0].fields["modules"] if x.typename == "nn.SpatialConvolution"]
    assert any((c.fields["kW"], c.fields["kH"], c.fields["padW"], c.fields["padH"]) == (1, 1, 0, 0) for c in convs) == (args[0] != args[1] or args[1] != args[2])
    # a cudnn.SpatialConvolution 1x1 as the reference's checkpoints name it
    for c in convs:
        c.typename = "cudnn.SpatialConvolution"
    assert np.array_equal(t7.to_model(raw)._flat_host(), m._flat_host())
