"""gpu: the VAE sampling layer (csrc/vae.hip) against float64 numpy (tests/vae_oracle.py) within the bounds tests/vae_paths.py derives from the
header's operation chains - every numeric check asserts max err / bound <= 1 and prints the ratio - its identities and limits, one step of
ganrev.train_vae's device loop against the split oracle, the fast loop against --compat, and the script end to end into ganrev.apply_r.
Outputs start from garbage (7)."""
import contextlib
import json
import os

import numpy as np
import pytest

import ganrev._lib as L
import vae_oracle as vo
import vae_paths as vp
from avgpool_oracle import SplitOracle, adopt_device_choices
from ganrev import device, synth, t7, train_vae, vae
from helpers import TOL, assert_close, assert_grads_close, param_segments
from test_vae_host import SHAPES, case, check_backward, check_forward, same_leaves

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def on_device(ctx, *arrays):
    ptrs = [None if a is None else ctx.upload(np.ascontiguousarray(a)) for a in arrays]
    try:
        yield ptrs
    finally:
        for p in ptrs:
            if p is not None:
                ctx.free(p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def sample_dev(ctx, h, eps, misalign=False, want=(True, True)):
    """-> dict(z, kl_rows, kl) through gr_vae_sample_dev; misalign: h_dev offset by 4 bytes (the scalar path whatever nd)"""
    B, nd = h.shape[0], h.shape[1] // 2
    table = np.concatenate([np.zeros(1, np.float32), h.reshape(-1)]) if misalign else h
    outs = (np.full((B, nd), 7, np.float32), np.full(B, 7, np.float32), np.full(1, 7.0))
    with on_device(ctx, table, eps, *outs) as (dh, de, dz, dr, dk):
        ctx.vae_sample_dev(dh + 4 if misalign else dh, de, B, nd, dz, dr if want[0] else None, dk if want[1] else None)
        return dict(z=ctx.download(dz, (B, nd)), kl_rows=ctx.download(dr, (B,)), kl=float(ctx.download(dk, (1,), np.float64)[0]))


def backward_dev(ctx, h, eps, gz, kl_weight, misalign=False):
    B, nd = gz.shape
    table = np.concatenate([np.zeros(1, np.float32), h.reshape(-1)]) if misalign else h
    with on_device(ctx, table, eps, gz, np.full((B, 2 * nd), 7, np.float32)) as (dh, de, dg, dout):
        ctx.vae_sample_backward_dev(dh + 4 if misalign else dh, de, dg, B, nd, kl_weight, dout)
        return ctx.download(dout, (B, 2 * nd))


# ------------------------------------------------------------------ 1. the kernels against the oracle
MEAN_EDGES = [(512, 1), (4096, 1), (4097, 1)]         # kl's chain: one full block, eight partials exactly, a ninth (1 and 513 rows are in SHAPES)


@pytest.mark.parametrize("B,nd", SHAPES + MEAN_EDGES)
def test_sampling_layer_matches_the_oracle_within_the_derived_bounds(ctx, B, nd):
    h, eps, gz = case(B, nd)
    name = f"({B}, {nd})"
    got = sample_dev(ctx, h, eps)
    check_forward(got, h, eps, name)
    check_backward(backward_dev(ctx, h, eps, gz, 0.75), h, eps, gz, 0.75, name)
    # once more with h_dev offset by 4 bytes: the scalar loads read the same values
    off = sample_dev(ctx, h, eps, misalign=True)
    check_forward(off, h, eps, name + " misaligned")
    goff = backward_dev(ctx, h, eps, gz, 0.75, misalign=True)
    check_backward(goff, h, eps, gz, 0.75, name + " misaligned")
    assert np.array_equal(bits(off["z"]), bits(got["z"])) and np.array_equal(bits(off["kl_rows"]), bits(got["kl_rows"])) and off["kl"] == got["kl"]
    assert np.array_equal(bits(goff), bits(backward_dev(ctx, h, eps, gz, 0.75)))


@pytest.mark.parametrize("B,nd", [(3, 5), (4, 16), (513, 100)])
def test_logvar_of_plus_and_minus_eighty(ctx, B, nd):
    h, eps, gz = case(B, nd, extreme=True)
    got = sample_dev(ctx, h, eps)
    assert np.isfinite(got["z"]).all() and np.isfinite(got["kl_rows"]).all() and np.isfinite(got["kl"])
    check_forward(got, h, eps, f"({B}, {nd}) logvar +-80")
    gh = backward_dev(ctx, h, eps, gz, 0.75)
    assert np.isfinite(gh).all()
    check_backward(gh, h, eps, gz, 0.75, f"({B}, {nd}) logvar +-80")


# ------------------------------------------------------------------ 2. identities
def test_null_eps_and_zero_weight(ctx):
    h, _, gz = case(5, 12)
    got = sample_dev(ctx, h, None)
    assert np.array_equal(got["z"], h[:, :12]), "eps null: z is mu"
    check_forward(got, h, None, "(5, 12) eps null")
    gh = backward_dev(ctx, h, None, gz, 0.0)
    assert np.array_equal(gh[:, :12], gz) and not gh[:, 12:].any(), "eps null, kl_weight 0: gmu is gz, glv is 0"
    check_backward(backward_dev(ctx, h, None, gz, 0.3), h, None, gz, 0.3, "(5, 12) eps null")


def test_kl_is_the_block_mean_of_the_rows(ctx):
    """kl[0] against the contract's own chain: the oracle's fp64 row sums differ from the kernel's only through exp, so their block mean is within
    kl_bound of the kernel's; and where every K_i is exact whatever exp's last bit (logvar = 0, mu = 0 or 2) the mean is exact, past a block edge too"""
    for B, nd in ((1025, 3), (513, 100)):
        h, eps, _ = case(B, nd)
        got = sample_dev(ctx, h, eps)
        ref = vo.forward(h, eps)
        assert abs(got["kl"] - vo.block_mean(ref["K"])) <= vp.kl_bound(ref)
        # the float rows, averaged the same way, are within their own rounding of it
        assert abs(got["kl"] - vo.block_mean(got["kl_rows"].astype(np.float64))) <= vp.U32 * float(np.abs(ref["K"]).mean()) * 1.01 + vp.kl_bound(ref)
    zero = sample_dev(ctx, np.zeros((700, 8), np.float32), None)
    assert zero["kl"] == 0.0 and not zero["kl_rows"].any()
    # integers: mu = 2, logvar = 0 gives 0.5 (4 + 1 - 1 - 0) = 2 per element, exactly, whatever exp's last bit: s = exp(0) = 1
    two = np.concatenate([np.full((1025, 7), 2, np.float32), np.zeros((1025, 7), np.float32)], axis=1)
    got = sample_dev(ctx, two, None)
    assert got["kl"] == 14.0 and (got["kl_rows"] == 14).all()


def test_null_outputs_are_accepted_and_left_alone(ctx):
    h, eps, _ = case(513, 16)
    full = sample_dev(ctx, h, eps)
    for want in ((False, False), (True, False), (False, True)):
        part = sample_dev(ctx, h, eps, want=want)
        assert np.array_equal(bits(part["z"]), bits(full["z"]))
        assert np.array_equal(bits(part["kl_rows"]), bits(full["kl_rows"])) if want[0] else (part["kl_rows"] == 7).all()
        assert part["kl"] == (full["kl"] if want[1] else 7.0)


def test_host_forms_give_the_bits_of_the_device_forms_and_two_runs_agree(ctx):
    for B, nd in ((3, 5), (513, 100)):
        h, eps, gz = case(B, nd)
        a, b = sample_dev(ctx, h, eps), sample_dev(ctx, h, eps)
        z, rows, kl = ctx.vae_sample_host(h, eps)
        for q, v in (("z", z), ("kl_rows", rows)):
            assert np.array_equal(bits(a[q]), bits(b[q])) and np.array_equal(bits(a[q]), bits(v)), q
        assert a["kl"] == b["kl"] == kl
        ga, gb = backward_dev(ctx, h, eps, gz, 0.2), backward_dev(ctx, h, eps, gz, 0.2)
        assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(ga), bits(ctx.vae_sample_backward_host(h, eps, gz, 0.2)))
    z, rows, kl = ctx.vae_sample_host(h, None, want_kl=False)
    assert rows is None and kl is None and np.array_equal(z, h[:, :nd])
    layer = vae.Sample(ctx)
    assert np.array_equal(bits(layer.forward(h, eps)), bits(a["z"])) and layer.kl == a["kl"]
    assert np.array_equal(bits(layer.backward(gz, 0.2)), bits(ga))


# ------------------------------------------------------------------ 3. limits
def test_limits_are_refused_by_name_and_nothing_is_launched(ctx):
    h, eps, gz = case(4, 8)
    assert ctx.VAE_MAX_ND == 256
    outs = (np.full((4, 8), 7, np.float32), np.full(4, 7, np.float32), np.full(1, 7.0), np.full((4, 16), 7, np.float32))
    with on_device(ctx, h, eps, gz, *outs) as (dh, de, dg, dz, dr, dk, dgh):
        for B, nd, status, text in ((4, 0, "GR_ERR_INVALID", "nd 0"), (4, 257, "GR_ERR_UNSUPPORTED", "nd 257"), (0, 8, "GR_ERR_INVALID", "B 0"),
                                    (-1, 8, "GR_ERR_INVALID", "B -1"), (1 << 31, 8, "GR_ERR_UNSUPPORTED", "B 2147483648")):
            with pytest.raises(L.GanrevError, match=f"gr_vae_sample_dev: {status}: gr_vae_sample_dev: .*{text}"):
                ctx.vae_sample_dev(dh, de, B, nd, dz, dr, dk)
            with pytest.raises(L.GanrevError, match=f"gr_vae_sample_backward_dev: {status}: gr_vae_sample_backward_dev: .*{text}"):
                ctx.vae_sample_backward_dev(dh, de, dg, B, nd, 0.5, dgh)
        for args in ((None, de, 4, 8, dz, dr, dk), (dh, de, 4, 8, None, dr, dk)):
            with pytest.raises(L.GanrevError, match="GR_ERR_INVALID: gr_vae_sample_dev: null pointer"):
                ctx.vae_sample_dev(*args)
        for args in ((None, de, dg, 4, 8, 0.5, dgh), (dh, de, None, 4, 8, 0.5, dgh), (dh, de, dg, 4, 8, 0.5, None)):
            with pytest.raises(L.GanrevError, match="GR_ERR_INVALID: gr_vae_sample_backward_dev: null pointer"):
                ctx.vae_sample_backward_dev(*args)
        ctx.synchronize()
        assert (ctx.download(dz, (4, 8)) == 7).all() and (ctx.download(dr, (4,)) == 7).all() and ctx.download(dk, (1,), np.float64)[0] == 7
        assert (ctx.download(dgh, (4, 16)) == 7).all()
        ctx.vae_sample_dev(dh, de, 4, 8, dz, dr, dk)                      # the context stays usable
        ctx.vae_sample_backward_dev(dh, de, dg, 4, 8, 0.5, dgh)
        got = dict(z=ctx.download(dz, (4, 8)), kl_rows=ctx.download(dr, (4,)), kl=float(ctx.download(dk, (1,), np.float64)[0]))
        check_forward(got, h, eps, "(4, 8) after the refusals")
        check_backward(ctx.download(dgh, (4, 16)), h, eps, gz, 0.5, "(4, 8) after the refusals")
    with pytest.raises(L.GanrevError, match="GR_ERR_UNSUPPORTED.*nd 257"):
        ctx.vae_sample_host(np.zeros((2, 514), np.float32))
    with pytest.raises(L.GanrevError, match="GR_ERR_UNSUPPORTED.*nd 257"):
        ctx.vae_sample_backward_host(np.zeros((2, 514), np.float32), None, np.zeros((2, 257), np.float32), 1.0)


# ------------------------------------------------------------------ 4. one VAE step against the split oracle
@pytest.mark.parametrize("criterion", ["mse", "bce"])
def test_vae_step_matches_split_oracle(oracle, ctx, conv_mode, criterion):
    """train_vae.DeviceLoop's forward, backward and Adam step with a fixed eps: SplitOracle over the encoder and over the decoder, vae_oracle
    between them; the bar of test_autoencoder_step_matches_split_oracle (tests/test_gpu_avgpool.py)"""
    dims, B, nd, w = (1, 32, 32), 4, 16, 0.5
    enc, dec = train_vae.build(dims, nd, 3)
    synth.init_params(enc, 3); synth.init_params(dec, 4)
    soe, sod = SplitOracle(oracle, enc, dims), SplitOracle(oracle, dec, (nd, 1, 1))
    soe.set_training(True); sod.set_training(True)
    x = synth.uniform((B,) + dims, 4, 0, 1)
    eps = synth.normal((B, nd), 5)
    loop = train_vae.DeviceLoop(enc, dec, dims, nd, B, L.Hyper(l1=0.0, l2=0.0, clamp=5.0), criterion, 1, w, 0)
    try:
        loop.load(x)
        loop.forward(0, eps_host=eps)
        h = ctx.download(loop.h, (B, 2 * nd))
        z = ctx.download(loop.z, (B, nd))
        out = ctx.download(loop.out, (B,) + dims)
        loss, kl = ctx.read_loss(loop.loss), ctx.read_loss(loop.kl)
        soe.forward(x)
        adopt_device_choices(enc, soe, B, 8, 1e-4, rel_flips=1e-4)
        rh = soe.forward(x)
        assert_close(h, rh, TOL, "h = (mu | logvar)")
        f = vo.forward(rh, eps)
        assert_close(z, f["z"], TOL, "z")
        assert abs(kl - f["kl"]) <= 1e-5 * max(1.0, abs(f["kl"])) + TOL * nd
        sod.forward(f["z"])
        adopt_device_choices(dec, sod, B, 8, 1e-4, rel_flips=1e-4)
        ref = sod.forward(f["z"])
        assert_close(out, ref, TOL, "decoder output")
        rloss, rg = oracle.bce(ref, x) if criterion == "bce" else oracle.mse(ref, x)
        assert abs(loss - rloss) <= 1e-5 * max(1.0, abs(rloss))
        loop.backward()
        soe.zero_grads(); sod.zero_grads()
        rgz = sod.backward(rg)
        soe.backward(vo.backward(rh, eps, rgz, w)["gh"])
        assert_grads_close(dec, dec._net.get_grads(), sod.grads, what="VAE decoder")
        assert_grads_close(enc, enc._net.get_grads(), soe.grads, what="VAE encoder")
        loop.step()
        for model, so, what in ((enc, soe, "encoder"), (dec, sod, "decoder")):
            theta = so.params.copy()
            m, v = np.zeros_like(theta), np.zeros_like(theta)
            oracle.penalty_clamp_adam(theta, so.grads.copy(), m, v, oracle.GoHyper(l1=0.0, l2=0.0, clamp=5.0), 1)
            # as in the autoencoder's test: the step is compared where the oracle's gradient is not rounding residue
            sig = np.abs(so.grads) > 1e-4 * max(1e-3, float(np.abs(so.grads).max()))
            assert_close(model._net.get_params()[sig], theta[sig], 2e-5, f"{what} parameters after one Adam step")
    finally:
        loop.close()


def test_logvar_rows_of_the_head_receive_exactly_zero(ctx):
    """kl_weight = 0 and eps null: glv is 0, so the gradient of the head Linear's logvar rows - weight and bias - is exactly 0"""
    dims, B, nd = (1, 32, 32), 4, 16
    enc, _ = train_vae.build(dims, nd, 6)
    synth.init_params(enc, 6)
    enc.device_net(dims)
    dm = device.DeviceModel(ctx, enc)
    x, gz = synth.uniform((B,) + dims, 7, 0, 1), synth.normal((B, nd), 8)
    try:
        with on_device(ctx, x, gz, np.full((B, 2 * nd), 7, np.float32)) as (dx, dg, dgh):
            dm.zero_grads()
            h = dm.forward(dx, B)
            ctx.vae_sample_backward_dev(h, None, dg, B, nd, 0.0, dgh)
            dm.backward(dgh, B, False)
            g = enc._net.get_grads()
    finally:
        dm.close()
    head = enc.leaves()[-1]
    (wlo, whi), (blo, bhi) = [(lo, hi) for mod, nm, lo, hi in param_segments(enc) if mod is head]
    gw, gb = g[wlo:whi].reshape(2 * nd, 512), g[blo:bhi]
    assert gw[:nd].any() and gb[:nd].any(), "the mu rows see gz"
    assert not gw[nd:].any() and not gb[nd:].any()


# ------------------------------------------------------------------ 5. the script
def _small_opts(save, extra=()):
    return ["--epochs", "1", "--N_epoch", "1", "--batchSize", "4", "--noiseDim", "16", "--colorSpace", "y", "--save", str(save), "--saveFreq", "1",
            "--klWeight", "0.1", "--quiet"] + list(extra)


def test_train_vae_fast_matches_compat(ctx, conv_mode, tmp_path):
    """one batch, the device loop against the closures over optim.adam, from identical state and with the same eps; the bar and the
    BatchNorm-bias residue rule of test_pretrain_fast_matches_compat (tests/test_gpu_avgpool.py)"""
    res = [train_vae.main(_small_opts(tmp_path / k, ["--conv-mode", conv_mode] + (["--compat"] if k == "compat" else []))) for k in ("fast", "compat")]
    assert abs(res[0]["last_loss"] - res[1]["last_loss"]) <= 1e-5 * max(1.0, abs(res[1]["last_loss"]))
    assert abs(res[0]["last_kl"] - res[1]["last_kl"]) <= 1e-5 * max(1.0, abs(res[1]["last_kl"]))
    for part in ("encoder", "decoder"):
        fast, compat = res[0][part], res[1][part]
        pf = (fast._flat_host() if fast._flat is None else fast._flat[0]).astype(np.float64)
        pc = compat._flat[0].astype(np.float64)
        d = np.abs(pf - pc)
        print(f"[train_vae fast vs compat] {conv_mode} {part}: max |dtheta| {d.max():.3e} ({'bit-identical' if d.max() == 0 else 'not bit-identical'})")
        leaves = compat.leaves()
        residue = np.zeros(d.size, bool)
        for mod, nm, lo, hi in param_segments(compat):
            i = leaves.index(mod)
            if nm == "bias" and i + 1 < len(leaves) and leaves[i + 1].typename.endswith("BatchNormalization") and not mod.typename.endswith("BatchNormalization"):
                residue[lo:hi] = True
        if conv_mode != "f16x3":
            assert d.max() == 0, "f32 / bf16x6: the host entry points run the same kernels as the device loop: bit-identical"
            continue
        assert d.max() <= 2.1e-3, d.max()
        r = d[~residue]
        assert np.median(r) <= 1e-7 and (r > 1e-5).mean() <= 1e-2, (np.median(r), (r > 1e-5).mean())


def test_train_vae_script_feeds_apply_r(ctx, tmp_path):
    from ganrev import apply_r
    nd, dims = 16, (3, 32, 32)
    res = train_vae.main(["--epochs", "2", "--N_epoch", "2", "--batchSize", "4", "--noiseDim", str(nd), "--save", str(tmp_path), "--quiet"])
    path, rpath = str(tmp_path / "vae_3x32x32_nd16.net"), str(tmp_path / "vae_r_3x32x32_nd16.net")
    assert res["path"] == path and res["reverser_path"] == rpath and os.path.isfile(path) and os.path.isfile(rpath)
    assert np.isfinite(res["last_loss"]) and res["last_kl"] >= 0
    ck, rk = t7.load_checkpoint(path), t7.load_checkpoint(rpath)
    assert "_unconverted" not in ck and "_unconverted" not in rk and int(ck["EPOCH"]) == 3
    same_leaves(ck["G"], res["decoder"])
    same_leaves(ck["E"], res["encoder"])
    assert all(m.running_mean.any() for m in ck["E"].leaves() if hasattr(m, "running_mean")), "the trained running statistics are saved"
    E, R = ck["E"], rk["R"]
    x = synth.synthetic_images(8, dims, 1 * 7919 + 2 * 3)                # the second epoch's first images
    E.evaluate(); R.evaluate()
    full = E.forward(x).copy()
    assert_close(R.forward(x), full[:, :nd], TOL, "R(x) against the mu half of E(x)")
    out = tmp_path / "out"
    apply_r.main(["--G", path, "--R", rpath, "--R_fixer", rpath, "--nbImages", "40", "--batchSize", "16", "--writeTo", str(out), "--quiet"])
    summary = json.load(open(out / "summary.json"))
    assert summary["dims"] == [3, 32, 32] and summary["noiseDim"] == nd
    assert np.load(out / "attributes.npy").shape == (40, nd)
    # the KL of the training images, in the VAE's own terms; the last chunk is shorter than the others
    dm = device.DeviceModel(ctx, E)
    xd = ctx.upload(x)
    try:
        mu, kl = vae.encode(ctx, dm, xd, 8, 3)
    finally:
        ctx.free(xd)
        dm.close()
    assert mu.shape == (8, nd) and kl.shape == (8,) and np.isfinite(kl).all() and (kl >= 0).all()
    assert_close(mu, full[:, :nd], TOL, "vae.encode's mu")
    ref = vo.forward(full, None)
    assert_close(kl, ref["kl_rows"], TOL * max(1.0, float(ref["kl_rows"].max())), "vae.encode's KL")
    assert not any(n.training for n in dm.nets), "the nets return to the mode they were in"
