"""cpu: the VAE oracle's own calculus (tests/vae_oracle.py), models.create_VAE_encoder, vae.mean_reverser, ganrev.train_vae's options, names and
schedule, and the t7 round trip of the two nets train_vae saves.  No GPU: nothing here calls the library's compute entry points."""
import numpy as np

import vae_oracle as vo
import vae_paths as vp
from ganrev import models, nn, t7, train_vae, vae

# (B, nd) of tests/test_gpu_vae.py: the scalar and the 16-byte paths, the wave edges, one row past a 512-row block, the nd limit
SHAPES = [(1, 1), (3, 5), (4, 16), (2, 63), (2, 64), (2, 65), (513, 100), (1025, 256)]


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(err).all() and np.isfinite(bound).all()
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def case(B, nd, seed=0, extreme=False):
    """(h, eps, gz) floats: mu in [-3, 3], logvar in [-6, 3] (extreme: +-80, alternating), eps ~ N(0, 1), gz ~ 0.1 N(0, 1)"""
    rng = np.random.default_rng(1000 * B + nd + seed)
    mu = rng.uniform(-3, 3, (B, nd))
    lv = rng.uniform(-6, 3, (B, nd))
    if extreme:
        lv = np.where((np.arange(B)[:, None] + np.arange(nd)[None, :]) % 2 == 0, 80.0, -80.0)
    h = np.concatenate([mu, lv], axis=1).astype(np.float32)
    return h, rng.standard_normal((B, nd)).astype(np.float32), (0.1 * rng.standard_normal((B, nd))).astype(np.float32)


def check_forward(got, h, eps, name):
    """got: dict(z, kl_rows, kl) from the code under test -> the err / bound ratios, each asserted <= 1"""
    ref = vo.forward(h, eps)
    mu, _ = vo.split(h)
    ratios = dict(z=worst(np.abs(got["z"].astype(np.float64) - ref["z64"]), vp.z_bound(ref, mu)),
                  kl_rows=worst(np.abs(got["kl_rows"].astype(np.float64) - ref["K"]), vp.kl_rows_bound(ref)),
                  kl=worst(abs(float(got["kl"]) - ref["kl"]), vp.kl_bound(ref)))
    print(f"{name}: forward err / bound " + ", ".join(f"{q} {v:.3g}" for q, v in ratios.items()))
    assert max(ratios.values()) <= 1, ratios
    return ratios


def check_backward(gh, h, eps, gz, kl_weight, name):
    ref = vo.backward(h, eps, gz, kl_weight)
    ratio = worst(np.abs(np.asarray(gh, np.float64) - ref["gh64"]), vp.gh_bound(ref, gz))
    print(f"{name}: backward err / bound gh {ratio:.3g}")
    assert ratio <= 1, ratio
    return ratio


def test_oracle_backward_matches_central_differences():
    """float64 throughout: the analytic gradient of 0.5 |z - target|^2 + kl_weight mean KL against central differences of the oracle's own loss"""
    B, nd, w = 3, 5, 0.37
    rng = np.random.default_rng(5)
    h = np.concatenate([rng.uniform(-2, 2, (B, nd)), rng.uniform(-3, 1.5, (B, nd))], axis=1)
    eps, target = rng.standard_normal((B, nd)), rng.standard_normal((B, nd))
    _, gz = vo.loss(h, eps, target, w)
    got = vo.backward(h, eps, gz, w)["gh64"]
    step = 1e-6
    for i in range(B):
        for j in range(2 * nd):
            hp, hm = h.copy(), h.copy()
            hp[i, j] += step; hm[i, j] -= step
            fd = (vo.loss(hp, eps, target, w)[0] - vo.loss(hm, eps, target, w)[0]) / (2 * step)
            assert abs(fd - got[i, j]) <= 1e-7 * max(1.0, abs(got[i, j])), (i, j, fd, got[i, j])
    # eps None is eps = 0: z = mu, and the logvar half sees the KL alone
    f = vo.forward(h.astype(np.float32), None)
    assert np.array_equal(f["z"], h[:, :nd].astype(np.float32))
    g = vo.backward(h, None, gz, 0.0)["gh64"]
    assert np.array_equal(g[:, :nd], gz) and not g[:, nd:].any()


def test_oracle_rounds_where_the_header_says_and_bounds_cover_its_own_float_outputs():
    for B, nd in SHAPES[:6] + [(513, 7)]:
        for extreme in (False, True):
            h, eps, gz = case(B, nd, extreme=extreme)
            f = vo.forward(h, eps)
            assert f["z"].dtype == np.float32 and f["kl_rows"].dtype == np.float32 and isinstance(f["kl"], float)
            assert (f["K"] >= -vp.rows_bound64(f)).all(), "a KL is not negative beyond its rounding"
            check_forward(f, h, eps, f"oracle ({B}, {nd})")
            check_backward(vo.backward(h, eps, gz, 0.01)["gh"], h, eps, gz, 0.01, f"oracle ({B}, {nd})")
    assert vo.block_mean(np.arange(1025.0)) == 512.0


def test_create_vae_encoder_is_the_g_encoder_under_another_head():
    dims, nd = (3, 32, 32), 12
    a, b = models.create_G_encoder(dims, nd, True, 4), models.create_VAE_encoder(dims, nd, True, 4)
    la, lb = a.leaves(), b.leaves()
    assert [m.typename for m in lb] == [m.typename for m in la[:-1]] and la[-1].typename == "nn.Tanh"
    assert isinstance(lb[-1], nn.Linear) and lb[-1].weight.shape == (2 * nd, 512) and la[-2].weight.shape == (nd, 512)
    for x, y in zip(la[:-2], lb[:-1]):                     # the trunk: the same layers; the same draws up to the first nn.Linear, which w_init redraws
        assert [p.shape for p in x.param_arrays()] == [q.shape for q in y.param_arrays()] and repr(x) == repr(y)
        if not isinstance(x, nn.Linear):
            assert all(np.array_equal(p, q) for p, q in zip(x.param_arrays(), y.param_arrays()))
    assert not lb[-1].bias.any() and lb[-1].weight.any()     # weight-init.lua's heuristic reaches the new head as it reaches the old one
    assert "no counterpart" in models.create_VAE_encoder.__doc__


def _encoder(dims=(1, 32, 32), nd=6, seed=2):
    enc = models.create_VAE_encoder(dims, nd, True, seed)
    rng = np.random.default_rng(seed)
    for m in enc.leaves():
        if hasattr(m, "running_mean"):
            m.running_mean[...] = rng.standard_normal(m.running_mean.shape)
            m.running_var[...] = rng.uniform(0.5, 2.0, m.running_var.shape)
    return enc


def same_leaves(a, b):
    assert [m.typename.replace("cudnn.", "nn.") for m in a.leaves()] == [m.typename.replace("cudnn.", "nn.") for m in b.leaves()]
    for x, y in zip(a.leaves(), b.leaves()):
        for p, q in zip(x.param_arrays(), y.param_arrays()):
            assert np.array_equal(p, q)
        if hasattr(x, "running_mean"):
            assert np.array_equal(x.running_mean, y.running_mean) and np.array_equal(x.running_var, y.running_var)


def test_mean_reverser_slices_the_head_and_copies_the_rest():
    nd = 6
    enc = _encoder(nd=nd)
    enc.evaluate()
    R = vae.mean_reverser(enc)
    le, lr = enc.leaves(), R.leaves()
    assert len(le) == len(lr) and all(x is not y for x, y in zip(le, lr))
    assert all(not m.train for m in R.listModules())
    for x, y in zip(le[:-1], lr[:-1]):
        assert x.typename == y.typename
        for p, q in zip(x.param_arrays(), y.param_arrays()):
            assert np.array_equal(p, q) and not np.shares_memory(p, q)
        if hasattr(x, "running_mean"):
            assert np.array_equal(x.running_mean, y.running_mean) and np.array_equal(x.running_var, y.running_var)
            assert not np.shares_memory(x.running_mean, y.running_mean)
    head, cut = le[-1], lr[-1]
    assert cut.weight.shape == (nd, 512) and np.array_equal(cut.weight, head.weight[:nd]) and np.array_equal(cut.bias, head.bias[:nd])
    # the host numpy forward of the cut Linear is the first half of the full one, bit for bit: each output is its own dot product
    x = np.random.default_rng(1).standard_normal((5, 512)).astype(np.float32)
    lin = lambda m: np.stack([np.array([np.dot(r, wrow) for wrow in m.weight], np.float32) + m.bias for r in x])
    assert np.array_equal(lin(cut), lin(head)[:, :nd])
    cut.weight[...] = 0
    assert head.weight[:nd].any(), "the reverser owns its arrays"


def test_train_vae_options_names_and_schedule():
    OPT = train_vae.parse([])
    assert (OPT.criterion, OPT.klWeight, OPT.klWarmup, OPT.noiseDim, OPT.batchSize, OPT.N_epoch, OPT.G_clamp, OPT.seed, OPT.compat) == \
        ("mse", None, 0, 100, 128, 30, 5.0, 1, False)
    assert (OPT.G_L1, OPT.G_L2, OPT.colorSpace, OPT.height, OPT.width, OPT.dataset, OPT.conv_mode) == (0.0, 0.0, "rgb", 32, 32, "NONE", "f16x3")
    assert train_vae.default_kl_weight((3, 32, 32)) == 1.0 / 3072 and train_vae.default_kl_weight((1, 64, 64)) == 1.0 / 4096
    assert train_vae.parse(["--criterion", "bce", "--klWeight", "0.5", "--klWarmup", "4"]).klWeight == 0.5
    assert train_vae.checkpoint_name((3, 32, 32), 100) == "vae_3x32x32_nd100.net"
    assert train_vae.reverser_checkpoint_name((1, 64, 48), 16) == "vae_r_1x64x48_nd16.net"
    w = 0.25
    assert [train_vae.kl_weight_at(w, 4, t) for t in (1, 2, 3, 4, 5, 6, 100)] == [0.0, 0.0625, 0.125, 0.1875, 0.25, 0.25, 0.25]
    assert [train_vae.kl_weight_at(w, 0, t) for t in (1, 2, 50)] == [w, w, w]
    assert train_vae.eps_seed(3, 7) == 3 * 1000003 + 7 and train_vae.eps_seed(3, 8) != train_vae.eps_seed(4, 7)


def test_encoder_and_reverser_round_trip_through_t7(tmp_path):
    nd = 6
    enc = _encoder(nd=nd)
    dec = models.create_G((1, 32, 32), nd, True, 3)
    OPT = train_vae.parse(["--noiseDim", str(nd), "--colorSpace", "y", "--save", str(tmp_path), "--quiet"])
    OPT.klWeight = train_vae.default_kl_weight((1, 32, 32))
    path, rpath = train_vae.save(OPT, enc, dec, (1, 32, 32), 1)
    assert path == str(tmp_path / "vae_1x32x32_nd6.net") and rpath == str(tmp_path / "vae_r_1x32x32_nd6.net")
    ck, rk = t7.load_checkpoint(path), t7.load_checkpoint(rpath)
    assert "_unconverted" not in ck and "_unconverted" not in rk and int(ck["EPOCH"]) == 2
    same_leaves(ck["E"], enc)
    same_leaves(ck["G"], dec)
    same_leaves(rk["R"], vae.mean_reverser(enc))
    for o in (ck["opt"], rk["opt"]):
        assert (int(o["noiseDim"]), int(o["height"]), int(o["width"]), o["colorSpace"], o["criterion"]) == (nd, 32, 32, "y", "mse")
        assert float(o["klWeight"]) == 1.0 / 1024
