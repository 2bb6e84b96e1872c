"""not-gpu: what tests/test_gpu_refine.py relies on, shown on the CPU - the case table of tests/refine_paths.py reaches every named feature, its
float64 reference tells a right input gradient / refinement loop from the degraded ones a wrong kernel would produce, and the inputs are
conditioned as the GPU tests assume."""
import numpy as np
import pytest
import torch

import refine_paths as rp


def test_the_table_reaches_every_named_feature():
    reached = set()
    for c in rp.CASES:
        for m in rp.modes_of(c):
            reached |= rp.features(c, m)
    missing = rp.ALL_FEATURES - rp.NOT_IN_TABLE - reached
    assert not missing, f"no case reaches {sorted(missing)}"
    assert not (rp.NOT_IN_TABLE & reached)
    assert {c.group for c in rp.CASES} == {"A", "B", "C"} and len({c.name for c in rp.CASES}) == len(rp.CASES)
    # both dgrad3 rules, both grouped-convolution routes, both frozen kernels on both sides of the pool
    assert rp.dgrad_family(rp.BY_NAME["B-up-conv-8-4"].stages[0], "f16x3", 3) == "conv3_split"
    assert rp.dgrad_family(rp.BY_NAME["B-up-conv-4-3"].stages[0], "f16x3", 3) == "conv3_f32"
    assert rp.dgrad_family(rp.BY_NAME["B-group-up-conv-default"].stages[0], "f16x3", 3) == "groupconv3_f32"
    assert rp.dgrad_family(rp.BY_NAME["B-group-up-conv-mfma"].stages[0], "bf16x6", 3, 1) == "groupconv3_mfma"
    assert rp.dgrad_family(rp.BY_NAME["B-group-up-conv-mfma"].stages[0], "f32", 3, 1) == "groupconv3_f32"
    pooled = {rp.frozen_label(st, c.B) for c in rp.CASES for st in c.stages if st.pool}
    assert pooled == {rp.FROZEN_VEC, rp.FROZEN_SCALAR}


def test_every_case_is_conditioned():
    for c in rp.CASES:
        d = rp.case_data(c.name)
        r = d["ref"]
        assert r["kink"] >= rp.KINK_GAP and r["pool_gap"] >= rp.POOL_GAP, c.name
        assert r["zmax"] <= rp.Z_MAX, (c.name, r["zmax"])
        assert np.abs(r["gin"]).max() > 0 and np.isfinite(r["gin"]).all()
        for k, (m, v) in enumerate(d["running"]):
            assert np.abs(m).max() > 0.05 and np.abs(v - 1).max() > 0.05, f"{c.name}: running statistics of BatchNorm {k} are trivial"
        if c.group == "A":
            assert 6.0 <= rp.c_bound(c) <= 128.0, (c.name, rp.c_bound(c))


def _rejected(case_name, degrade):
    """the largest |degraded - reference| of gradInput over the bound the GPU test of that case applies, element by element"""
    c = rp.BY_NAME[case_name]
    d = rp.case_data(case_name)
    ref = d["ref"]["gin"]
    bad = rp.reference(c.descs, c.dims, d, degrade=degrade)["gin"]
    err = np.abs(bad - ref)
    if c.group == "A":
        bound = rp.c_bound(c) * rp.U * np.abs(ref)
        return float((err / np.maximum(bound, 1e-300)).max())
    return float(err.max() / (rp.GRAD_RTOL * np.abs(ref).max()))


@pytest.mark.parametrize("case,degrade", [
    ("A-bn-relu-3x5x7", "no_scale"), ("A-bn-relu-3x5x7", "batch_stats"), ("B-conv-sbn-elu-max", "no_scale"), ("B-conv-sbn-elu-max", "batch_stats"),
    ("B-linear-bn-relu", "batch_stats"), ("A-leaky-drop-8x8", "no_mask"), ("A-always-on-drop-8x8", "no_mask"), ("A-prelu-sdrop-avg-8x16", "no_mask"),
    ("A-bn-elu-max-8x8", "no_pool_scatter"), ("B-conv-sbn-elu-max", "no_pool_scatter"), ("A-bn-relu-odd-max-5x7", "no_pool_scatter")])
def test_the_reference_rejects_a_degraded_input_gradient(case, degrade):
    ratio = _rejected(case, degrade)
    print(f"{case} with {degrade}: {ratio:.3g} x the bound")
    assert ratio > 10.0
    assert _rejected(case, None) == 0.0


def test_the_loop_is_conditioned_and_float32_stays_within_a_quarter_of_the_bar():
    li = rp.loop_inputs()
    r64 = li["r64"]
    assert len(r64["grads"]) == rp.LOOP["steps"]
    for t, g in enumerate(r64["grads"], 1):          # no Adam step decided by rounding
        assert np.abs(g).min() >= rp.G_COND * np.abs(g).max(), f"step {t}: min |g| / max |g| = {np.abs(g).min() / np.abs(g).max():.3e}"
    assert (r64["best"] < r64["first"]).all()
    nd = rp.LOOP["nd"]
    f32 = rp.build(li["descs"], (nd, 1, 1), li["params"], li["running"], dtype=torch.float32)
    r32 = rp.refine_loop(f32, li["images"], li["z0"], rp.LOOP["steps"], rp.LOOP["lr"], dtype=torch.float32)
    dz = float(np.abs(r32["z"] - r64["z"]).max())
    print(f"loop seed {li['seed']}: min |g| / max |g| over all steps {li['cond']:.3e}; float32 emulation max |z - z64| = {dz:.3e} = {dz / rp.NOISE_TOL:.4f} of the bar")
    assert dz <= rp.NOISE_TOL / 4
    # chunking cannot matter: evaluate()-mode G couples no two rows
    f64 = rp.build(li["descs"], (nd, 1, 1), li["params"], li["running"])
    half = rp.refine_loop(f64, li["images"][:4], li["z0"][:4], rp.LOOP["steps"], rp.LOOP["lr"])
    assert np.abs(half["z"] - r64["z"][:4]).max() <= 1e-12


def test_the_reference_rejects_a_degraded_loop():
    li = rp.loop_inputs()
    nd = rp.LOOP["nd"]
    f64 = rp.build(li["descs"], (nd, 1, 1), li["params"], li["running"])
    # epsilon inside the bias correction: sqrt(v / bc2) + eps against sqrt(v) / sqrt(bc2) + eps / sqrt(bc2) - visible because eps / sqrt(bc2) is a
    # few per cent of these gradients
    inside = rp.refine_loop(f64, li["images"], li["z0"], rp.LOOP["steps"], rp.LOOP["lr"], eps_inside=True)
    d = float(np.abs(inside["z"] - li["r64"]["z"]).max())
    print(f"epsilon inside the bias correction: max |z - z64| = {d:.3e}")
    assert d > 2 * rp.NOISE_TOL
    # a missed best-keeping: steps large enough to overshoot, so that some row's last z is not its best
    kept = rp.refine_loop(f64, li["images"], li["z0"], rp.LOOP["steps"], 0.5)
    last = rp.refine_loop(f64, li["images"], li["z0"], rp.LOOP["steps"], 0.5, keep_best=False)
    assert (kept["best"] <= kept["first"]).all()
    assert (last["best"] > kept["best"]).any() and float(np.abs(last["z"] - kept["z"]).max()) > 2 * rp.NOISE_TOL


def test_adam_rows_mirror_is_optim_adam_in_float32():
    """refine_paths.adam_rows in float32 against the kernel's operation order written out in numpy float32 (csrc/elem.hip adam_one)"""
    rng = np.random.default_rng(1)
    z0, g = rng.standard_normal(40).astype(np.float32), (rng.standard_normal(40) * 0.3).astype(np.float32)
    z, m, v = torch.tensor(z0.copy()), torch.zeros(40), torch.zeros(40)
    nz, nm, nv = z0.copy(), np.zeros(40, np.float32), np.zeros(40, np.float32)
    f = np.float32
    for t in (1, 2, 3):
        rp.adam_rows(z, torch.tensor(g), m, v, t, 0.01)
        step = f(-(0.01 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
        nm = nm * f(0.9) + f(1.0 - 0.9) * g
        nv = nv * f(0.999) + (f(1.0 - 0.999) * g) * g
        nz = nz + (step * nm) / (np.sqrt(nv) + f(1e-8))
        assert np.array_equal(z.numpy(), nz) and np.array_equal(m.numpy(), nm) and np.array_equal(v.numpy(), nv)
