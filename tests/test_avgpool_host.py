"""not-gpu: nn.SpatialAveragePooling(2,2,2,2), the builders that use it (models.lua:57-102, 213-270, 339-383), their Torch7
checkpoints, the split oracle the GPU tests hold the device to (pinned here against float64 PyTorch), and the option / lookup
logic of ganrev.pretrain_g and ganrev.train's pretrained G."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ganrev._lib as L
from ganrev import models, nn, pretrain_g, synth, t7, train
from avgpool_oracle import SplitOracle, avgpool_forward
from helpers import assert_close
from torch_twin import Twin

AVGPOOL2 = 17


def test_module_desc_and_geometry():
    m = nn.SpatialAveragePooling(2, 2, 2, 2)
    assert m.typename == "nn.SpatialAveragePooling"
    assert m.desc((5, 9, 7)) == ([(L.AVGPOOL2, 0, 0, 0, 0.0, 0)], (5, 4, 3))
    assert L.AVGPOOL2 == AVGPOOL2
    for args in [(2, 2), (3, 3, 2, 2), (2, 2, 2, 2, 1, 1), (2, 2, 1, 1)]:
        with pytest.raises(L.GanrevError):
            nn.SpatialAveragePooling(*args)


def _fields_equal(a, b):
    assert a.typename == b.typename
    assert set(a.fields) == set(b.fields), (a.typename, set(a.fields) ^ set(b.fields))
    for k, v in a.fields.items():
        w = b.fields[k]
        if k == "modules":               # nn.Copy (host <-> device transfer) is dropped on loading, as cudnn.convert(model, nn) would
            v = [m for m in v if m.typename != "nn.Copy"]
            assert len(v) == len(w)
            for x, y in zip(v, w):
                _fields_equal(x, y)
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, np.asarray(w)), (a.typename, k)
        elif not isinstance(v, t7.TorchObject):
            assert v == w, (a.typename, k, v, w)


@pytest.mark.parametrize("make", [
    lambda: (lambda s: (s.add(nn.SpatialConvolution(3, 8)), s.add(nn.ReLU()), s.add(nn.SpatialAveragePooling(2, 2, 2, 2)), s)[-1])(nn.Sequential()),
    lambda: models.create_D_default((3, 32, 32)),
    lambda: models.create_D_facegen((3, 32, 32)),
    lambda: pretrain_g.build((3, 32, 32), 100, 1).get(2)])
def test_torch7_round_trip(tmp_path, make):
    model = make()
    path = str(tmp_path / "m.net")
    t7.save_checkpoint(path, G=model, opt={"colorSpace": "rgb"})
    ck = t7.load_checkpoint(path)
    assert "_unconverted" not in ck                    # before GR_AVGPOOL2 such trees stayed unconverted
    back = ck["G"]
    _fields_equal(t7.from_model(model), t7.from_model(back))
    raw = t7.load(path)["G"]
    pools = [m for m in raw.fields["modules"] if m.typename == "nn.SpatialAveragePooling"]
    for p in pools:
        assert {k: p.fields[k] for k in ("kW", "kH", "dW", "dH", "padW", "padH", "ceil_mode", "count_include_pad", "divide")} == \
            dict(kW=2, kH=2, dW=2, dH=2, padW=0, padH=0, ceil_mode=False, count_include_pad=True, divide=True)
    assert np.array_equal(back._flat_host(), model._flat_host())


def _types(model):
    return [m.typename for m in model.leaves()]


def test_builders_follow_models_lua():
    conv, cbn, relu = "cudnn.SpatialConvolution", "nn.SpatialBatchNormalization", "cudnn.ReLU"
    enc = models.create_G_encoder((3, 32, 32), 100)
    assert _types(enc) == [conv, cbn, relu, "nn.SpatialAveragePooling", conv, cbn, relu, "nn.SpatialMaxPooling",
                           conv, cbn, relu, "nn.SpatialMaxPooling", "nn.View", "nn.Linear", "nn.BatchNormalization", relu,
                           "nn.Linear", "nn.Tanh"]
    sizes = [3 * 16 * 9 + 16, 2 * 16, 16 * 32 * 9 + 32, 2 * 32, 32 * 64 * 9 + 64, 2 * 64, 64 * 4 * 4 * 512 + 512, 2 * 512, 512 * 100 + 100]
    assert enc._param_count() == sum(sizes) == 600932
    assert all(float(np.abs(m.bias).max()) == 0 for m in enc.leaves() if m.typename == conv)     # weight-init.lua:70-72
    sc, pr, sd, ap = "nn.SpatialConvolution", "nn.PReLU", "nn.SpatialDropout", "nn.SpatialAveragePooling"
    d = models.create_D_default((3, 32, 32))
    assert _types(d) == [sc, pr, sc, pr, sd, sc, pr, sd, ap, sc, pr, sd, ap, sc, pr, sd, ap, "nn.View", "nn.Linear", pr,
                         "nn.Dropout", "nn.Linear", "nn.Sigmoid"]
    assert [m.p for m in d.leaves() if m.typename in (sd, "nn.Dropout")] == [0.25] * 4 + [0.5]
    f = models.create_D_facegen((3, 32, 32))
    assert _types(f) == [sc, pr, sd, ap] * 4 + ["nn.View", "nn.Linear", pr, "nn.Dropout", "nn.Linear", pr, "nn.Dropout", "nn.Linear", "nn.Sigmoid"]
    assert [m.p for m in f.leaves() if m.typename in (sd, "nn.Dropout")] == [0.2] * 4 + [0.5, 0.5]
    assert [m.weight.shape[1] for m in f.leaves() if m.typename == "nn.Linear"] == [512 * 2 * 2, 512, 512]
    assert all(m.weight.size == 1 for m in f.leaves() if m.typename == pr)        # nn.PReLU(nil, nil, true): one slope


class AvgTwin(Twin):
    """torch_twin.Twin plus GR_AVGPOOL2 (F.avg_pool2d), with gradInput; float64"""

    def forward(self, x):
        x = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
        self.x = x
        B, bi, h = x.shape[0], 0, x
        for li, (d, p) in enumerate(zip(self.descs, self.params)):
            k = d[0]
            if k == AVGPOOL2:
                h = F.avg_pool2d(h, 2, 2)
            elif k == 1:
                h = F.conv2d(h, p[0], p[1], padding=1)
            elif k == 16:
                h = F.prelu(h, p[0])
            elif k == 13:
                h = F.linear(h.reshape(B, -1), p[0], p[1])
            elif k == 2:
                rm, rv = self.bn_running[bi]; bi += 1
                h = F.batch_norm(h, rm, rv, p[0], p[1], self.training, 0.1, 1e-5)
            elif k == 4:
                h = F.relu(h)
            elif k == 7:
                h = torch.tanh(h)
            elif k == 8:
                if self.training:
                    h = h * torch.tensor(self.masks[li].astype(np.float64)).reshape(h.shape) * (1.0 / (1.0 - d[4]))
            elif k == 9:
                h = h * (torch.tensor(self.masks[li].astype(np.float64)).reshape(B, h.shape[1], 1, 1) if self.training else (1.0 - d[4]))
            elif k == 10:
                h = F.max_pool2d(h, 2, 2)
            elif k == 12:
                h = h.reshape((B, d[1]) if (d[2] <= 1 and d[3] <= 1) else (B, d[1], d[2], d[3]))
            else:
                raise AssertionError(f"kind {k}")
        self.out = h
        return h.detach().numpy()

    def backward(self, gout):
        flat_p = [q for p in self.params if p is not None for q in p]
        gs = torch.autograd.grad(self.out, [self.x] + flat_p, torch.tensor(np.asarray(gout, np.float64)), allow_unused=True)
        return gs[0].numpy(), np.concatenate([(g if g is not None else torch.zeros_like(q)).reshape(-1).numpy() for g, q in zip(gs[1:], flat_p)])


def test_avgpool_arithmetic_is_thnns():
    x = synth.normal((2, 3, 5, 7), 1)
    v = x[:, :, :4, :6]
    want = ((((np.float32(0) + v[:, :, 0::2, 0::2]) + v[:, :, 0::2, 1::2]) + v[:, :, 1::2, 0::2]) + v[:, :, 1::2, 1::2]) / np.float32(4)
    assert np.array_equal(avgpool_forward(x), want)


@pytest.mark.parametrize("training", [True, False])
def test_split_oracle_matches_float64_torch(oracle, training):
    """the composition the GPU tests use: oracle parts chained around numpy average pools, against one float64 evaluation"""
    model = nn.Sequential()
    for mod in [nn.SpatialConvolution(3, 8), nn.SpatialBatchNormalization(8), nn.ReLU(), nn.SpatialAveragePooling(2, 2, 2, 2),
                nn.Dropout(0.5), nn.SpatialConvolution(8, 8), nn.PReLU(), nn.SpatialDropout(0.25), nn.SpatialAveragePooling(2, 2, 2, 2),
                nn.SpatialConvolution(8, 8), nn.SpatialBatchNormalization(8), nn.ReLU(), nn.SpatialMaxPooling(2, 2),
                nn.View(32), nn.Linear(32, 5), nn.Tanh()]:
        model.add(mod)
    synth.init_params(model, 3)
    dims, B = (3, 18, 19), 3                         # odd width: floor at every pool
    so = SplitOracle(oracle, model, dims)
    so.set_training(training)
    descs, index = model._descs(dims)
    masks = {}
    for m in model.leaves():
        if m.typename in ("nn.Dropout", "nn.SpatialDropout"):
            keep = synth.bernoulli_keep((so.mask_size(m, B),), index[id(m)], m.p)
            so.set_mask(m, keep); masks[index[id(m)]] = keep
    twin = AvgTwin(descs, dims, model._flat_host(), [(m.running_mean, m.running_var) for m in model.leaves() if hasattr(m, "running_mean")],
                   training, masks)
    x = synth.uniform((B,) + dims, 4, -1, 1)
    ref = twin.forward(x)
    out = so.forward(x)
    assert_close(out, ref, 1e-5, "forward")
    if not training:
        return                                       # (evaluate(): the oracle has no backward)
    gy = synth.normal(ref.shape, 5)
    so.zero_grads()
    gin = so.backward(gy)
    tgin, tg = twin.backward(gy)
    assert_close(gin, tgin, 1e-5 * max(1.0, float(np.abs(tgin).max())), "gradInput")
    assert_close(so.grads, tg, 1e-4 * max(1.0, float(np.abs(tg).max())), "parameter gradients")


def test_pretrain_options():
    o = pretrain_g.parse([])
    assert (o.save, o.saveFreq, o.batchSize, o.N_epoch, o.G_L1, o.G_L2, o.G_clamp, o.noiseDim, o.colorSpace, o.height, o.width, o.seed) == \
        ("logs", 30, 128, 30, 0.0, 0.0, 5.0, 100, "rgb", 32, 32, 1)
    assert (o.data, o.compat, o.conv_mode, o.quiet, o.epochs) == ("", False, "f16x3", False, 1)
    assert pretrain_g.image_dims(pretrain_g.parse(["--colorSpace", "y", "--height", "64", "--width", "48"])) == (1, 64, 48)
    assert pretrain_g.checkpoint_name((3, 32, 32), 100) == "g_pretrained_3x32x32_nd100.net"
    t = train.parse([])
    assert t.G_pretrained_dir == "logs" and t.nopretraining is False


def test_train_finds_the_pretrained_G(tmp_path):
    dims = (3, 32, 32)
    opt = train.parse(["--G_pretrained_dir", str(tmp_path), "--noiseDim", "16", "--quiet"])
    assert train.pretrained_G_path(opt, dims) is None
    dec = models.create_G(dims, 16)
    t7.save_checkpoint(str(tmp_path / "g_pretrained_3x32x32_nd16.net"), G=dec, opt={"colorSpace": "rgb"}, EPOCH=2)
    assert train.pretrained_G_path(opt, dims) == os.path.join(str(tmp_path), "g_pretrained_3x32x32_nd16.net")
    assert train.pretrained_G_path(opt, (1, 32, 32)) is None                            # another geometry, another file
    G = train.create_or_load_G(opt, dims)
    assert np.array_equal(G._flat_host(), dec._flat_host()) and all(m.train for m in G.listModules())
    opt.nopretraining = True
    assert train.pretrained_G_path(opt, dims) is None
