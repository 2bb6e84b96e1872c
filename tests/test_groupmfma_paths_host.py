"""CPU checks of tests/groupmfma_paths.py: the restated constants, support rule and dispatch rule are those of csrc/groupmfma.hip and
csrc/net.hip; the case table reaches every loop step and edge the restated launch arithmetic distinguishes; with the default tuning key
every grouped shape the older tests run keeps its fp32 kernels; the per-element float64 bound accepts float32 emulations of both split
arithmetics in kernel order on every case and rejects degraded ones; the weight gradient's constant is twice the measured."""
import functools
import math
import os
import re

import numpy as np
import pytest

import generic_paths as gp
import groupmfma_paths as gm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan-reverser_amd", "csrc")

REQUIRED_FEATURES = [
    # forward / data gradient kernel: the wave loop over tile pairs, ragged tiles, both store forms, both staging forms
    "fwd a wave takes a second round of tiles", "fwd odd tile count: a round's second tile is past the end", "fwd waves without a tile",
    "fwd staging loop: a partial round (some threads stage nothing)", "fwd staging loop runs more than once", "fwd border loop runs twice",
    "fwd ragged last 16-pixel tile", "fwd a 16-pixel tile spans rows that are not aligned", "fwd width exactly two pixel tiles",
    "fwd 16-byte stores", "fwd scalar stores", "fwd staged behind the up-sampling (four cells per source pixel)", "fwd plain staging",
    "fwd 1x1 source: every tap but the centre block padded", "LDS at its largest (32 x 32)",
    "dgrad a wave takes a second round of tiles", "dgrad odd tile count: a round's second tile is past the end", "dgrad waves without a tile",
    "dgrad staging loop: a partial round (some threads stage nothing)", "dgrad staging loop runs more than once", "dgrad border loop runs twice",
    "dgrad<up>: tiles of 4 source pixels x their 2 x 2 block", "dgrad<up>: ragged last tile (source pixels % 4 != 0)",
    "dgrad plain with 16-byte stores", "dgrad plain with scalar stores", "a second group's weights and planes", "G odd",
    # weight gradient: splits, the image loop, the k steps of a wave, the k tail, the pitch, the LDS aliasing
    "wgrad per_split >= 2 and last split shorter", "wgrad used < splits", "wgrad one image per split",
    "wgrad a split walks several images (per-image scale-back, planes staged anew)", "wgrad a wave takes a second k step",
    "wgrad a wave takes ten k steps", "wgrad waves without a k step", "wgrad k tail beyond the plane (H P % 32 != 0)",
    "wgrad A fragment partly outside its row (W % 8 != 0)", "wgrad A fragments wholly inside or outside (W % 8 == 0)", "wgrad pitch 40 (W + 2 <= 40 < W + 8)",
    "wgrad pitch 8", "wgrad planes smaller than the cross-wave scratch", "wgrad planes larger than the cross-wave scratch",
    "wgrad staged behind the up-sampling", "wgrad plain staging",
    # the f16x3 scales
    "f16x3: a tile of zeros (scale 1)", "f16x3: tiles 2^60 apart in one batch",
]


def test_every_required_feature_is_reached():
    reached = {}
    for c in gm.CASES:
        for k, v in c.features().items():
            if v:
                reached.setdefault(k, []).append(c.name)
    assert len(set(REQUIRED_FEATURES)) == len(REQUIRED_FEATURES) and len(gm.BY_NAME) == len(gm.CASES) == 7
    for f in REQUIRED_FEATURES:
        print(f"{f}: {', '.join(reached.get(f, []))}")
    known = {k for c in gm.CASES for k in c.features()}
    assert set(REQUIRED_FEATURES) == known, sorted(set(REQUIRED_FEATURES) ^ known)
    missing = [f for f in REQUIRED_FEATURES if f not in reached]
    assert not missing, f"no case reaches: {missing}"


def test_the_table_is_the_issues_table():
    """(B, G, H x W, up) as the issue lists them, and what the launch formulas give for them, by hand from the sources"""
    assert [(c.name, c.B, c.G, c.H, c.W, c.up) for c in gm.CASES] == [
        ("gm_mini", 3, 2, 8, 8, True), ("gm_odd", 5, 3, 5, 7, False), ("gm_plane_max", 2, 1, 32, 32, False), ("gm_g4_plane", 17, 2, 32, 32, True),
        ("gm_tiny", 1, 1, 2, 2, True), ("gm_band", 2, 2, 3, 32, False), ("gm_zero_and_scales", 3, 1, 8, 8, True)]
    f = gm.conv_launch(5, 3, 5, 7, False, False, 2)
    assert (f["grid"], f["tiles"], f["rounds"], f["cells"], f["lds"], f["vec"], f["stage_items"]) == ((3, 5), 3, 1, 63, 4032, False, 70)
    f = gm.conv_launch(2, 1, 32, 32, False, False, 3)
    assert (f["tiles"], f["rounds"], f["cells"], f["lds"]) == (64, 8, 1156, 110976)
    d = gm.conv_launch(17, 2, 32, 32, True, True, 2)
    assert (d["tiles"], d["Ho"], d["Wo"], d["stage_items"], d["vec"]) == (64, 16, 16, 2048, False)
    d = gm.conv_launch(1, 1, 2, 2, True, True, 2)
    assert (d["tiles"], d["Ho"] * d["Wo"]) == (1, 1)
    w = gm.wgrad_launch(17, 2, 32, 32, True, 3)
    assert (w["grid"], w["per"], w["last_images"], w["P"], w["ksteps"], w["PL"], w["lds"]) == ((2, 9), 2, 1, 40, 40, 1376, 132096)
    w = gm.wgrad_launch(2, 2, 3, 32, False, 2)
    assert (w["P"], w["ksteps"], w["PL"], w["planes_bytes"], w["lds"]) == (40, 4, 224, 14336, 36864)
    w = gm.wgrad_launch(5, 3, 5, 7, False, 2)
    assert (w["grid"], w["P"], w["ksteps"]) == ((3, 5), 16, 3)
    assert gm.wgrad_launch(1, 1, 2, 2, True, 2)["ksteps"] == 1


def test_restated_constants_are_the_sources():
    src = open(os.path.join(CSRC, "groupmfma.hip")).read()
    for k, v in dict(GM_PLANES=gm.GM_PLANES, GM_MAX_HW=gm.GM_MAX_HW, GM_KSTEPS=gm.GM_KSTEPS, GM_MAX_SPLITS=gm.GM_MAX_SPLITS,
                     g_group_mfma_min_tiles=gm.DEFAULT_MIN_TILES).items():
        m = re.search(rf"\b{k} = (\d+)\b", src)
        assert m and int(m.group(1)) == v, (k, v, m and m.group(1))
    assert "GM_RED_FLOATS = 4 * 9 * 256;" in src and gm.GM_RED_FLOATS == 4 * 9 * 256
    # the support rule, the split rule, the pitch / step / plane arithmetic and the LDS sizes
    assert ("return G >= 1 && Cin == GM_PLANES * G && Cout == GM_PLANES * G && H >= 1 && H <= GM_MAX_HW && W >= 1 && W <= GM_MAX_HW && "
            "(!up || (H % 2 == 0 && W % 2 == 0));") in src
    assert "return B < GM_MAX_SPLITS ? B : GM_MAX_SPLITS;" in src
    assert "per = (B + splits - 1) / splits, used = (B + per - 1) / per;" in src
    assert "P = round_up(W + 2, 8), ksteps = (H * P + 31) / 32;" in src and "ksteps * 32 + 2 * P + 16}" in src
    assert "return (size_t)nterm * (H + 2) * (W + 2) * 32;" in src
    assert "ntiles = up_out ? (HWo + 3) / 4 : (HW + 15) / 16;" in src and "t0 = 2 * wave; t0 < ntiles; t0 += 8" in src
    assert set(re.findall(r'KtScope kt\("([^"]+)"', src)) == set(gm.MFMA_LABELS)
    group = open(os.path.join(CSRC, "group.hip")).read()
    assert set(re.findall(r'KtScope kt\("(groupconv3[^"]+|group_wgrad[^"]+)"', group)) == set(gm.FP32_LABELS)
    assert gm.GM_MAX_SPLITS <= gp.GC_MAX_SPLITS              # groupconv3_workspace_bytes holds the MFMA launch's partials too
    net = open(os.path.join(CSRC, "net.hip")).read()
    assert ("return n->ctx->conv_mode != 0 && s.kind == ST_GROUPCONV && groupconv3_mfma_supported(s.Cin, s.Cout, s.groups, s.H, s.W, s.up) && "
            "(long)B * s.groups >= g_group_mfma_min_tiles;") in net
    assert '"group_mfma_min_tiles")) { gr::g_group_mfma_min_tiles = value;' in net


def test_lds_and_workspace_on_a_grid():
    """every supported shape fits the LDS of a workgroup in both arithmetics; the workspace net.hip sizes covers what the launch writes"""
    worst = 0
    for H in range(1, 33):
        for W in range(1, 33):
            for nt in (2, 3):
                worst = max(worst, gm.conv_launch(1, 1, H, W, False, False, nt)["lds"], gm.wgrad_launch(1, 1, H, W, False, nt)["lds"])
    print(f"largest LDS allocation {worst} bytes")
    assert worst == gm.wgrad_launch(1, 1, 32, 32, False, 3)["lds"] == 132096 <= gm.LDS_LIMIT
    for B in (1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 256, 512):
        for G in (1, 2, 3, 32):
            m = gm.wgrad_launch(B, G, 8, 8, True, 2)
            assert m["used"] <= m["splits"] <= gm.GM_MAX_SPLITS and m["used"] * m["per"] >= B and (m["used"] - 1) * m["per"] < B and 1 <= m["last_images"] <= m["per"]
            assert m["written"] <= m["ws_floats"] == gm.workspace_floats(B, 16 * G, 16 * G, G)
    for args in ((16, 16, 1, 33, 8, False), (16, 16, 1, 8, 33, False), (16, 32, 1, 8, 8, False), (22, 38, 2, 18, 17, False), (9, 15, 3, 36, 32, True),
                 (32, 32, 2, 6, 7, True), (16, 16, 1, 0, 8, False)):
        assert not gm.supported(*args), args
    for args in ((16, 16, 1, 1, 1, False), (512, 512, 32, 32, 32, True), (48, 48, 3, 5, 7, False)):
        assert gm.supported(*args), args


def test_default_key_keeps_the_older_tests_on_the_fp32_kernels():
    """generic_paths' gc_* cases and test_gpu_g4.py's grouped shapes (B <= 10) record the fp32 labels under the default key in every mode;
    create_G4's stage at B = 16 takes the MFMA labels"""
    for mode in ("f32",) + gm.MODES:
        for c in gp.CASES:
            if c.kind == "gc":
                assert gm.dispatch(mode, c.B, c.Cin, c.Cout, c.G, c.H, c.W, c.up) == set(gp.GC_LABELS) == set(gm.FP32_LABELS)
        for B in range(1, 11):                      # create_G4's grouped convolution, the miniature's (2 planes) and groupconv3_alone's shapes
            for Cin, Cout, G, H, W, up in ((512, 512, 32, 32, 32, True), (6, 6, 3, 8, 8, True), (12, 18, 3, 6, 8, True), (8, 8, 2, 5, 7, False)):
                assert gm.dispatch(mode, B, Cin, Cout, G, H, W, up) == set(gm.FP32_LABELS)
        want = gm.FP32_LABELS if mode == "f32" else gm.MFMA_LABELS
        assert gm.dispatch(mode, 16, 512, 512, 32, 32, 32, True) == set(want)
        assert gm.dispatch(mode, 15, 512, 512, 32, 32, 32, True) == set(gm.FP32_LABELS)
    assert gm.DEFAULT_MIN_TILES == 512 > 10 * 32
    for c in gm.CASES:
        assert c.labels("f16x3", 1) == set(gm.MFMA_LABELS) and c.labels("f32", 1) == set(gm.FP32_LABELS) and c.labels("f16x3", gm.DEFAULT_MIN_TILES) == set(gm.FP32_LABELS)


# ---------------------------------------------------------------- the bound and its teeth
@functools.lru_cache(maxsize=None)
def _emulated(name, kind):
    return gm.emulate(name, kind)


def _worst(name, mode, em, keys=("out", "gin", "gw")):
    ref = gm.reference(name, mode)
    return {k: float(gm.ratio(em[k], ref[k][0], ref[k][1]).max()) for k in keys}


@pytest.mark.parametrize("mode", gm.MODES)
@pytest.mark.parametrize("name", [c.name for c in gm.CASES])
def test_bound_accepts_the_emulation_in_kernel_order(name, mode):
    ref = gm.reference(name, mode)
    for k, (r, bound, A) in ref.items():
        assert r.shape == bound.shape == A.shape and np.all(np.isfinite(r)) and np.all(np.isfinite(bound)) and np.all(bound >= 0)
        assert np.all((bound > 0) | (A == 0)), f"{name} {k}: an element with operands but without a bound"
    r = _worst(name, mode, _emulated(name, mode))
    print(name, mode, {k: round(v, 3) for k, v in r.items()})
    assert all(v <= 1.0 for v in r.values()), r


def test_constants_are_twice_the_measured():
    """the weight gradient's c: largest err / (U A) of the emulations over every case, the f16x3 allowance C16 M taken off; and the forward /
    data gradient emulations stay within half of conv_paths.C_MODE, the constant they borrow"""
    for mode in gm.MODES:
        worst, conv = (0.0, ""), (0.0, "")
        for c in gm.CASES:
            ref, em = gm.reference(c.name, mode), _emulated(c.name, mode)
            r, _, A = ref["gw"]
            ok = A > 0
            q = np.abs(em["gw"].astype(np.float64) - r)[ok] / (gm.U * A[ok]) - gm.f16_slack(c.name, mode)[ok]
            if float(q.max()) > worst[0]:
                worst = (float(q.max()), c.name)
            for k in ("out", "gin"):
                r, bound, A = ref[k]
                ok = A > 0
                extra = (bound[ok] / gm.U - gm.cp.C_MODE[mode] * A[ok]) / A[ok]          # C16 M and the bias, in units of U A
                q = float((np.abs(em[k].astype(np.float64) - r)[ok] / (gm.U * A[ok]) - extra).max())
                if q > conv[0]:
                    conv = (q, f"{c.name} {k}")
        print(f"{mode}: weight gradient {worst[0]:.2f} ({worst[1]}), forward / data gradient {conv[0]:.2f} ({conv[1]}) of {gm.cp.C_MODE[mode]}")
        assert abs(worst[0] - gm.MEASURED_WGRAD[mode]) <= 0.02 * gm.MEASURED_WGRAD[mode], (mode, worst, gm.MEASURED_WGRAD[mode])
        assert gm.C_WGRAD[mode] == math.ceil(2 * gm.MEASURED_WGRAD[mode])
        assert 2 * conv[0] <= gm.cp.C_MODE[mode], (mode, conv)


# case, arithmetic whose bound is applied, degraded emulation, the tensors it must push out of the bound
DEGRADED = [
    ("gm_mini", "f16x3", "f16x3_without_x1w0", ("out", "gin", "gw")),
    ("gm_odd", "f16x3", "f16x3_without_x1w0", ("out", "gin", "gw")),
    ("gm_mini", "bf16x6", "bf16x6_without_order2", ("out", "gin", "gw")),
    ("gm_odd", "bf16x6", "bf16x6_without_order2", ("out", "gin", "gw")),
    # one scale for the whole tensor: the 2^-30 image's gradOutput falls below fp16's range beside the 2^30 one and its gradInput is lost
    # (its forward output is within rounding of its bias, which the bound's extra term covers, and its weight-gradient share is 2^-120 of the sum)
    ("gm_zero_and_scales", "f16x3", "f16x3_scale_per_tensor", ("gin",)),
]


@pytest.mark.parametrize("name,mode,kind,keys", DEGRADED, ids=[f"{n}-{k}" for n, _, k, _ in DEGRADED])
def test_bound_rejects_degraded_arithmetic(name, mode, kind, keys):
    r = _worst(name, mode, gm.emulate(name, kind), keys)
    print(name, kind, {k: f"x{v:.3g}" for k, v in r.items()})
    for k, v in r.items():
        assert v > 1.0, f"{name}: the bound accepts {kind} in {k} (max err / bound {v:.3f})"


def test_zero_tile_gives_exactly_the_bias():
    """the emulation's statement of the kernels' rule: a tile of zeros takes scale 1, its output is the bias, its gradients are zero"""
    d, em = gm.inputs("gm_zero_and_scales"), _emulated("gm_zero_and_scales", "f16x3")
    assert np.array_equal(em["out"][1], np.broadcast_to(d["b"][:, None, None], em["out"][1].shape)) and not np.any(em["gin"][1])
