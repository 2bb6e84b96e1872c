"""CPU: models.create_G4 (reference models.lua:145-194) as a module tree - structure, parameter count, what weight-init.lua leaves of
it, the Torch7 checkpoint round trip with nn.Reshape - and how it is compiled: as one grouped net (nn.bundle_plan: descriptors, the parameter permutation, the BatchNorm map) or, with
`concat.bundle = False`, as 32 branch nets and one tail net.  Nothing here touches the GPU: modules are built, never run."""
import numpy as np
import pytest

import ganrev._lib as L
from ganrev import models, nn, t7, train

BRANCH = ["nn.Linear", "nn.PReLU", "nn.Linear", "nn.BatchNormalization", "nn.PReLU", "nn.Reshape", "nn.SpatialUpSamplingNearest",
          "cudnn.SpatialConvolution", "nn.SpatialBatchNormalization", "nn.PReLU"]


def _types(seq):
    return [m.typename for m in seq.modules]


def _conv(m):
    return (m.nInputPlane, m.nOutputPlane, m.kW, m.kH)


@pytest.mark.parametrize("dims,nd", [((1, 32, 32), 32), ((3, 32, 32), 100), ((3, 64, 64), 100)])
def test_module_tree_equals_models_lua(dims, nd):
    G = models.create_G4(dims, nd)
    assert _types(G) == ["nn.Copy", "nn.Concat", "cudnn.SpatialConvolution", "nn.SpatialBatchNormalization", "nn.PReLU",
                         "cudnn.SpatialConvolution", "nn.Sigmoid", "nn.Copy"]
    concat = G.modules[1]
    assert concat.dimension == 2 and len(concat.modules) == 32
    for seq in concat.modules:
        assert seq.typename == "nn.Sequential" and _types(seq) == BRANCH
        lin1, _, lin2, bn1, _, reshape, _, conv, bn2, _ = seq.modules
        assert lin1.weight.shape == (16, nd) and lin2.weight.shape == (16 * 16 * 16, 16) and bn1.nFeature == 16 * 16 * 16
        assert reshape.sizes == (16, 16, 16) and _conv(conv) == (16, 16, 3, 3) and bn2.nFeature == 16
        assert all(p.weight.shape == (1,) and p.weight[0] == np.float32(0.25) for p in seq.modules if p.typename == "nn.PReLU")
    # startHeight / startWidth are computed and not used (models.lua:152-153): 512 x 32 x 32 joins the tail whatever `dimensions` says
    assert _conv(G.modules[2]) == (512, 64, 3, 3) and G.modules[3].nFeature == 64 and _conv(G.modules[5]) == (64, dims[0], 3, 3)
    d = (nd, 1, 1)
    for m in concat.modules[0].leaves():
        _, d = m.desc(d)
    assert d == (16, 32, 32)


@pytest.mark.parametrize("dims,nd", [((1, 32, 32), 32), ((3, 32, 32), 100)])
def test_parameter_count_and_order(dims, nd):
    G = models.create_G4(dims, nd)
    C, Ct = dims[0], 32 * 16
    branch = (nd * 16 + 16) + 1 + (16 * 4096 + 4096) + 2 * 4096 + 1 + (16 * 16 * 9 + 16) + 2 * 16 + 1
    tail = (Ct * 64 * 9 + 64) + 2 * 64 + 1 + (64 * C * 9 + C)
    assert G.children() is None and not G._is_graph() and len(G._param_chunks()) == 1          # the bundle: a plain net to every caller
    G.modules[1].bundle = False                                                                   # the parts route
    flat, grads = G.getParameters()
    assert flat.size == grads.size == 32 * branch + tail
    # branch-major: branch j owns [j * branch, (j + 1) * branch), the tail what is left; each is one compiled net
    chunks = G._param_chunks()
    assert [(lo, hi) for _, lo, hi in chunks] == [(j * branch, (j + 1) * branch) for j in range(32)] + [(32 * branch, 32 * branch + tail)]
    assert [type(p).__name__ for p in G.parts()] == ["Concat", "Sequential"] and G._is_graph() and G.children() is not None
    b7 = G.modules[1].modules[7]
    assert np.shares_memory(b7.modules[0].weight, flat) and np.array_equal(flat[7 * branch:7 * branch + nd * 16], b7.modules[0].weight.ravel())
    assert flat[7 * branch + nd * 16 + 16] == np.float32(0.25)                     # the first slope sits behind the first Linear
    tw = G.modules[2].weight
    assert np.array_equal(flat[32 * branch:32 * branch + tw.size], tw.ravel())


def test_weight_init_leaves_what_weight_init_lua_leaves():
    """weight-init.lua:52-72 walks the TOP-LEVEL modules only and re-draws nn.SpatialConvolution / nn.Linear by exact class name: of G4
    it sees an nn.Concat (no match, no bias) and two cudnn.SpatialConvolution (no match: only their bias is zeroed).  Every branch
    keeps its constructor draw, biases included."""
    G = models.create_G4((1, 32, 32), 32, seed=3)
    for conv in (G.modules[2], G.modules[5]):
        bound = 1.0 / np.sqrt(9 * conv.nInputPlane)                                 # the constructor's uniform(-stdv, stdv)
        assert not conv.bias.any() and 0.8 * bound < np.abs(conv.weight).max() <= bound
    assert not G.modules[3].bias.any()
    for seq in G.modules[1].modules:
        lin1, _, lin2, bn1, _, _, _, conv, bn2, _ = seq.modules
        for m, fan_in in ((lin1, 32), (lin2, 16), (conv, 9 * 16)):
            bound = 1.0 / np.sqrt(fan_in)
            assert m.bias.any() and np.abs(m.bias).max() <= bound and 0.8 * bound < np.abs(m.weight).max() <= bound
        assert 0 <= bn1.weight.min() and bn1.weight.max() <= 1 and bn1.weight.std() > 0.2 and not bn1.bias.any() and not bn2.bias.any()
    # one process-wide generator: no two branches start out identical, the same seed gives the same model
    first = [seq.modules[0].weight for seq in G.modules[1].modules]
    assert all(not np.array_equal(first[0], w) for w in first[1:])
    assert np.array_equal(models.create_G4((1, 32, 32), 32, seed=3)._flat_host(), G._flat_host())
    assert not np.array_equal(models.create_G4((1, 32, 32), 32, seed=4)._flat_host(), G._flat_host())


def _signature(m):
    name = m.typename.replace("cudnn.", "nn.")
    if hasattr(m, "modules"):
        return (name, getattr(m, "dimension", None), [_signature(x) for x in m.modules if x.typename != "nn.Copy"])
    extra = {k: getattr(m, k) for k in ("nInputPlane", "nOutputPlane", "kW", "kH", "nFeature", "sizes") if hasattr(m, k)}
    return (name, extra, [a.tobytes() for a in m.param_arrays()] + [getattr(m, k).tobytes() for k in ("running_mean", "running_var") if hasattr(m, k)])


def test_t7_round_trip_with_reshape():
    G = models.create_G4((3, 32, 32), 8, seed=5)
    for x in G.leaves():
        if hasattr(x, "running_mean"):
            x.running_mean[...] = np.linspace(-1, 1, x.nFeature); x.running_var[...] = np.linspace(0.5, 2, x.nFeature)
        if x.typename == "nn.PReLU":
            x.weight[...] = 0.1 + 0.01 * (id(x) % 17)
    data = t7.dumps(t7.from_model(G))
    back = t7.to_model(t7.load(data))
    assert _signature(back) == _signature(G)                                         # (the nn.Copy brackets are dropped on loading, as always)
    assert np.array_equal(back._flat_host(), G._flat_host())
    again = t7.dumps(t7.from_model(back))
    assert t7.dumps(t7.from_model(t7.to_model(t7.load(again)))) == again
    # the fields Torch7's nn.Reshape keeps: size and batchsize as torch.LongStorage, nelement as a number
    raw = t7.load(data)
    reshape = raw.fields["modules"][1].fields["modules"][0].fields["modules"][5]
    assert reshape.typename == "nn.Reshape" and isinstance(reshape.fields["size"], t7.Storage) and isinstance(reshape.fields["batchsize"], t7.Storage)
    assert list(reshape.fields["size"]) == [16, 16, 16] and list(reshape.fields["batchsize"])[1:] == [16, 16, 16] and reshape.fields["nelement"] == 4096
    assert reshape.fields["size"].dtype == np.int64
    # through a checkpoint file, as train.lua:256 writes it: G converts, nothing is left unconverted
    ck = t7.load_checkpoint(t7.dumps({"G": t7.from_model(G), "opt": {"noiseDim": 8}}))
    assert "_unconverted" not in ck and isinstance(ck["G"], nn.Sequential) and np.array_equal(ck["G"]._flat_host(), G._flat_host())


def test_reshape_is_a_view_with_its_own_name():
    r = nn.Reshape(2, 4, 4)
    assert r.typename == "nn.Reshape" and r.desc((32, 1, 1)) == ([(L.VIEW, 2, 4, 4, 0.0, 0)], (2, 4, 4)) and r.leaves() == [r]
    assert nn.Reshape(12).desc((3, 2, 2)) == ([(L.VIEW, 12, 1, 1, 0.0, 0)], (12, 1, 1))
    with pytest.raises(L.GanrevError, match=r"nn.Reshape\(2, 4, 4\): input has 30 elements"):
        r.desc((30, 1, 1))
    raw = t7.from_model(nn.Sequential().add(r)).fields["modules"][0]
    raw.fields["batchMode"] = False
    with pytest.raises(ValueError, match="batchMode"):
        t7.to_model(raw)


def test_single_net_paths_refuse_a_model_of_several_nets_by_name():
    """forwardBatchedDev, apply_r.embed_dev and train_r's DeviceTrainer drive ONE gr_net: G4 is 33, and says so before anything is compiled"""
    G = models.create_G4((1, 32, 32), 8)
    G.modules[1].bundle = False
    with pytest.raises(L.GanrevError, match="runs as 33 nets"):
        G.device_net((8,))
    assert all(ch._net is None for ch, _, _ in G._param_chunks())


def test_bundle_plan_of_g4():
    nd, nb = 32, 32
    G = models.create_G4((1, 32, 32), nd)
    descs, perm, bn_map = nn.bundle_plan(G, (nd,))
    assert descs == [(L.LINEAR, nd, nb * 16, 0, 0.0, 0), (L.PRELU, nb, 0, 0, 0.0, 0), (L.GROUPLINEAR, nb * 16, nb * 4096, nb, 0.0, 0),
                     (L.BN, nb * 4096, 0, 0, 0.0, 0), (L.PRELU, nb, 0, 0, 0.0, 0), (L.VIEW, nb * 16, 16, 16, 0.0, 0), (L.UPSAMPLE2, 0, 0, 0, 0.0, 0),
                     (L.GROUPCONV3, nb * 16, nb * 16, nb, 0.0, 0), (L.BN, nb * 16, 0, 0, 0.0, 0), (L.PRELU, nb, 0, 0, 0.0, 0),
                     (L.CONV3, 512, 64, 0, 0.0, 0), (L.BN, 64, 0, 0, 0.0, 0), (L.PRELU, 0, 0, 0, 0.0, 0), (L.CONV3, 64, 1, 0, 0.0, 0), (L.SIGMOID, 0, 0, 0, 0.0, 0)]
    n = G._param_count()
    assert perm.dtype == np.int64 and perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n))
    # the tree filled with its own indices: every tensor of the net is the branches' tensors one after another, layer by layer
    flat, _ = G.getParameters()
    flat[...] = np.arange(n)                             # (exact in float32 below 2^24)
    assert n < 2 ** 24
    net = flat[perm]
    at = 0
    branches = [[m for m in b.modules if m.leaves()] for b in G.modules[1].modules]
    for p in range(len(branches[0])):
        for q in range(len(branches[0][p].param_arrays())):
            for br in branches:
                a = br[p].param_arrays()[q]
                assert np.array_equal(net[at:at + a.size], a.ravel()), (p, q)
                at += a.size
    for m in G.modules[2:]:
        for a in m.param_arrays():
            assert np.array_equal(net[at:at + a.size], a.ravel())
            at += a.size
    assert at == n
    # the grouped Linear's weight is [b][a / G]: branch j's [4096][16] matrix at rows [4096 j, 4096 (j + 1))
    w_at = nd * 16 * nb + 16 * nb + nb
    assert np.array_equal(net[w_at:w_at + nb * 4096 * 16].reshape(nb, 4096, 16)[5], branches[5][2].weight)
    assert bn_map == [list(range(0, 64, 2)), list(range(1, 64, 2)), [64]]
    # the compile decision
    assert G.children() is None and G._descs((nd, 1, 1))[0] == descs and np.array_equal(G._perm((nd, 1, 1)), perm)
    G.modules[1].bundle = False
    assert nn.bundle_plan(G, (nd,)) is None and len(G.children()) == 2


def _branchy(make_branch, nb=3, tail=True):
    model, cat = nn.Sequential(), nn.Concat(2)
    for j in range(nb):
        cat.add(make_branch(j))
    model.add(cat)
    if tail:
        model.add(nn.Linear(6 * nb, 2))
    return model


def test_bundle_plan_declines():
    ok = _branchy(lambda j: nn.Sequential().add(nn.Linear(4, 6)).add(nn.PReLU()))
    descs, perm, bn_map = nn.bundle_plan(ok, (4,))
    assert descs == [(L.LINEAR, 4, 18, 0, 0.0, 0), (L.PRELU, 3, 0, 0, 0.0, 0), (L.LINEAR, 18, 2, 0, 0.0, 0)] and bn_map == [] and ok.children() is None
    assert nn.bundle_plan(models.create_D2((1, 16, 16)), (1, 16, 16)) is None
    assert nn.bundle_plan(models.createResidual(4, 2, 4), (4, 8, 8)) is None
    cases = {
        "unequal width": _branchy(lambda j: nn.Sequential().add(nn.Linear(4, 6 if j else 5)).add(nn.PReLU()), tail=False),
        "dropout": _branchy(lambda j: nn.Sequential().add(nn.Linear(4, 6)).add(nn.Dropout(0.5))),
        "first module no Linear": _branchy(lambda j: nn.Sequential().add(nn.View(4)).add(nn.Linear(4, 6))),
        "another activation": _branchy(lambda j: nn.Sequential().add(nn.Linear(4, 6)).add(nn.ReLU())),
        "one branch": _branchy(lambda j: nn.Sequential().add(nn.Linear(4, 6)), nb=1),
        "nested container": _branchy(lambda j: nn.Sequential().add(nn.Sequential().add(nn.Linear(4, 6)))),
    }
    for name, model in cases.items():
        assert nn.bundle_plan(model, (4,)) is None and model.children() is not None, name
    other = nn.Sequential().add(nn.Linear(4, 4)).add(ok.modules[0])                # a layer in front of the Concat
    assert nn.bundle_plan(other, (4,)) is None
    outer = nn.Sequential().add(nn.Linear(4, 4)).add(ok)                           # a bundle inside a larger model is one part of it
    assert outer._is_graph() and [type(p).__name__ for p in outer.parts()] == ["Sequential", "Sequential"] and outer.parts()[1] is ok


def test_train_options():
    assert train.parse([]).G_model == "create_G3"                                    # models.create_G (models.lua:201-203)
    assert train.parse(["--G_model", "create_G4"]).G_model == "create_G4"
    with pytest.raises(SystemExit):
        train.parse(["--G_model", "create_G2"])
    for bad in (["--height", "64"], ["--width", "16"]):
        with pytest.raises(SystemExit, match="create_G4 paints 32x32 images only"):
            train.main(["--G_model", "create_G4", "--epochs", "1", "--N_epoch", "1", "--batchSize", "4", "--quiet"] + bad)
