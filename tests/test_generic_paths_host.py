"""CPU checks of tests/generic_paths.py: the case table reaches every loop iteration and tile edge of the 1x1, grouped and 5x5 weight-gradient
launches that the restated arithmetic distinguishes; the mirror names only KtScope labels of the sources; the restated split and workspace
arithmetic is consistent; the per-element float64 bound accepts float32 emulations in kernel order and rejects subtly degraded ones; the
constants are twice what those emulations measure."""
import functools
import math
import os
import re

import numpy as np
import pytest

import generic_paths as gp

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan-reverser_amd", "csrc")

# One entry per branch no test ran before this table (first block of each kind), then the ones the older tests already reach.
REQUIRED_FEATURES = [
    # conv1x1_wgrad_kernel: the pipelined loop's second iteration, the hand-over, ragged last chunks, a second input-axis tile
    "c1_wgrad_chunks_per_split >= 2", "c1_wgrad_chunks_per_split >= 3", "c1_wgrad ragged last chunk inside a multi-chunk split",
    "c1_wgrad last split shorter: one ragged chunk behind multi-chunk splits", "c1_wgrad multi-chunk with vec tile loads",
    "c1_wgrad multi-chunk with scalar tile loads", "c1_wgrad split count capped by c1_split_cap", "c1_wgrad input-axis tiles >= 2",
    "c1_reduce 16-block and tail",
    # conv1x1_kernel as data gradient (WK = false): MB 4, gridDim.y > 1; and the forward's edges
    "c1_dgrad_MB == 4", "c1_dgrad_MB == 4 and grid_y >= 2", "c1_fwd_MB == 4 and grid_y >= 2", "c1_fwd_MB == 4 and the last block holds one plane",
    "c1_fwd_k_chunks >= 3 with an odd tail (kn < 32)", "c1_dgrad_k_chunks >= 3 with an odd tail (kn < 32)", "c1_fwd_k_chunks >= 2 with an even tail",
    "c1_vec staging with HW below a tile", "c1_scalar staging and MB == 1",
    # already reached before
    "c1_fwd_MB == 1", "c1_fwd_MB == 2", "c1_fwd_MB == 4", "c1_dgrad_MB == 1", "c1_vec staging", "c1_scalar staging", "c1_fwd_K odd and below one chunk",
    "c1_dgrad_K odd and below one chunk", "c1_pixel tile crosses an image boundary", "c1_ragged last pixel tile", "c1_wgrad_chunks_per_split == 1",
    "c1_wgrad last split ragged with single-chunk splits", "c1_wgrad output-axis tiles >= 2", "c1_wgrad ragged channel tiles on both axes", "c1_reduce tail only",
    # grouped Linear: the k0 loop's second step, block_sum_256 on reused sh, the second batch tiles
    "gl_k_chunks >= 2 with a ragged last", "gl_dgrad a second block_sum_256 round on reused sh", "gl_fwd batch tiles >= 2 with a ragged last (GL_BT)",
    "gl_dgrad batch tiles >= 2 with a ragged last (GL_DB)", "gl_fwd an output block of 256 holds a group boundary", "gl_k exactly one full chunk",
    "gl_dgrad thread stride over Mg above 256", "gl_dgrad Mg below 256",
    # grouped convolution: ragged second register chunks, per_split 2, used < splits, the up-sampled data gradient over two tiles
    "gc_fwd ragged second GC_OC chunk", "gc_dgrad ragged second GC_CI chunk", "gc_wgrad ragged GC_WO chunks (>= 2)", "gc_per_split >= 2 and last split shorter",
    "gc used < splits", "gc_wgrad thread loop over pixels runs twice", "gc_dgrad<1> (up-sampled) with input-pixel tiles >= 2", "gc_dgrad<0>", "gc_fwd pixel tiles >= 2",
    "gc odd width",
    # multi-slope PReLU: parts > 1, the PM_PARTS cap with its grid-stride loop, the 4096-workgroup cap
    "pm 1 < parts < PM_PARTS", "pm parts capped at PM_PARTS with the grid-stride loop", "pm_blocks capped at 4096", "pm L not a multiple of 256",
    # 5x5 weight gradient: b += gridDim.z steps, blockIdx.y > 0
    "k5_wgrad image loop steps (b += gridDim.z) in some splits only", "k5_wgrad blockIdx.y >= 1 with a ragged tail", "k5_wgrad blockIdx.x >= 1 with a ragged tail",
    "k5_wgrad ragged 8x16 tiles on both axes",
]


def test_every_required_feature_is_reached():
    reached = {}
    for c in gp.CASES:
        for k, v in c.features().items():
            if v:
                reached.setdefault(k, []).append(c.name)
    assert len(set(REQUIRED_FEATURES)) == len(REQUIRED_FEATURES) and len(gp.BY_NAME) == len(gp.CASES) == 13
    for f in REQUIRED_FEATURES:
        print(f"{f}: {', '.join(reached.get(f, []))}")
    missing = [f for f in REQUIRED_FEATURES if f not in reached]
    assert not missing, f"no case reaches: {missing}"
    known = {k for c in gp.CASES for k in c.features()}
    assert set(REQUIRED_FEATURES) <= known, sorted(set(REQUIRED_FEATURES) - known)


def test_the_table_is_the_issues_table():
    """what the launch formulas give for the named shapes, by hand from the sources"""
    w = gp.c1_wgrad(5 * 324, 324, 260, 260)
    assert (w["cap"], w["klen"], w["splits"], w["last_pixels"], w["reduce16"], w["reduce_tail"], w["vec"]) == (40, 64, 26, 20, 1, 10, True)
    w = gp.c1_wgrad(25 * 49, 49, 520, 520)
    assert (w["cap"], w["klen"], w["splits"], w["chunks"], w["last_pixels"], w["last_chunks"], w["vec"]) == (12, 128, 10, 4, 73, 3, False)
    f = gp.c1_gemm(25 * 49, 49, 520, 520)
    assert (f["MB"], f["grid_y"], f["k_chunks"], f["kn_last"]) == (4, 5, 17, 8)
    w = gp.c1_wgrad(144, 16, 130, 129)
    assert (w["in_tiles"], w["out_tiles"], w["splits"], w["last_pixels"]) == (3, 3, 5, 16)
    f = gp.c1_gemm(150, 25, 67, 33)
    assert (f["MB"], f["k_chunks"], f["kn_last"], f["vec"]) == (2, 3, 4, False) and gp.c1_gemm(150, 25, 33, 67)["MB"] == 4
    m = gp.gl_launch(11, 111, 300, 3)
    assert (m["Kg"], m["Mg"], m["fwd_grid"], m["dgrad_grid"], m["k_chunks"], m["k_tail"]) == (37, 100, (2, 2), (3, 3), 3, 5)
    m = gp.gc_launch(19, 22, 38, 2, 18, 17, False)
    assert (m["Cg"], m["Og"], m["oc_chunks"], m["ci_chunks"], m["wo_chunks"], m["per"], m["used"], m["last_images"], m["pixel_rounds"]) == (11, 19, 2, 2, 3, 2, 10, 1, 2)
    m = gp.gc_launch(17, 9, 15, 3, 36, 32, True)
    assert (m["dgrad_grid"][0], m["per"], m["used"], m["last_images"]) == (2, 2, 9, 1)
    assert gp.pm_launch(5, 6, 23 * 19, 3)["parts"] == 5
    m = gp.pm_launch(8, 6, 64 * 65, 3)
    assert (m["total"], m["parts_wanted"], m["parts"], m["grid_stride"]) == (66560, 65, 64, True)
    m = gp.pm_launch(3, 2, 840 * 840, 2)
    assert m["n"] > 4096 * 1024 and m["blocks"] == 4096
    m = gp.k5_wgrad(70, 20, 68, 9, 18)
    assert (m["grid"], m["two_image_splits"], m["tiles"]) == ((2, 2, 64), 6, (2, 2))


def _ktscope_names():
    """the labels the three sources give their KtScope timers: plain string literals, and convk_direct's names, which it builds from a
    literal prefix and its template arguments"""
    names = set()
    for f in gp.SOURCES:
        src = open(os.path.join(CSRC, f)).read()
        names |= set(re.findall(r'KtScope kt\("([^"]+)"', src))
        if f == "convk.hip":
            cot = re.search(r"constexpr int COT = (\d+);", src).group(1)
            ks = re.search(r"constexpr int KC_KS = (\d+);", src).group(1)
            assert "convk_direct<5>" in src and "nm_bwd = nm + \"(dgrad)\"" in src
            for base, last in re.findall(r'nm = "(convk_direct\w*_kernel)<" \+ std::to_string\(K\) \+ ", " \+ std::to_string\(COT\) \+ (", " \+ std::to_string\(KC_KS\) \+ ">"|", 1>")', src):
                nm = f"{base}<5, {cot}, {ks if 'KC_KS' in last else 1}>"
                names |= {nm, nm + "(dgrad)"}
    return names


def test_mirror_names_only_ktscope_labels_of_the_sources():
    names = _ktscope_names()
    assert names == set(gp.UNIVERSE), f"sources only: {sorted(names - gp.UNIVERSE)}; mirror only: {sorted(gp.UNIVERSE - names)}"
    seen = set()
    for B in (1, 3, 17, 64, 70, 300):
        for Cin, Cout in ((1, 1), (5, 7), (32, 33), (64, 65), (130, 129), (520, 520)):
            for H, W in ((1, 1), (4, 4), (5, 5), (9, 18), (32, 32)):
                for kind in ("c1", "k5"):
                    seen |= gp.Case("grid", kind, B, Cin, Cout, H, W).labels()
        for G, Cg, Og in ((1, 5, 7), (3, 37, 100), (2, 16, 300)):
            seen |= gp.Case("grid", "gl", B, G * Cg, G * Og, G=G).labels()
            seen |= gp.Case("grid", "gc", B, G * Cg, G * Og, 6, 8, G=G, up=True).labels() | gp.Case("grid", "gc", B, G * Cg, G * Og, 5, 7, G=G).labels()
        seen |= gp.Case("grid", "pm", B, 6, 6, 5, 7, G=3).labels()
    assert seen <= gp.UNIVERSE, sorted(seen - gp.UNIVERSE)
    for c in gp.CASES:
        assert c.labels() <= gp.UNIVERSE and c.labels()


def test_restated_constants_are_the_sources():
    """every constant of the mirror, read from the .hip files"""
    want = {"conv1x1.hip": dict(C1_NT=gp.C1_NT, C1_KC=gp.C1_KC, C1_MAX_WGS=gp.C1_MAX_WGS, C1_MAX_SPLITS=gp.C1_MAX_SPLITS),
            "group.hip": dict(GL_BT=gp.GL_BT, GL_KC=gp.GL_KC, GL_DB=gp.GL_DB, GC_OC=gp.GC_OC, GC_CI=gp.GC_CI, GC_WO=gp.GC_WO, GC_MAX_SPLITS=gp.GC_MAX_SPLITS,
                              PM_PARTS=gp.PM_PARTS),
            "convk.hip": dict(KW_CI=gp.KW_CI, KW_CO=gp.KW_CO, KW_ROWS=gp.KW_ROWS, KC_TILE=gp.KC_TILE)}
    for f, consts in want.items():
        src = open(os.path.join(CSRC, f)).read()
        for k, v in consts.items():
            m = re.search(rf"\b{k} = (\d+)\b", src)
            assert m and int(m.group(1)) == v, (f, k, v, m and m.group(1))
    src = open(os.path.join(CSRC, "group.hip")).read()
    assert "b > 4096 ? 4096 : b" in src and gp.PM_MAX_BLOCKS == 4096
    assert "return B < 64 ? B : 64;" in open(os.path.join(CSRC, "convk.hip")).read() and gp.CONVK_MAX_SPLITS == 64


def test_split_arithmetic_and_workspaces_on_a_grid():
    """splits * klen covers N with no empty split, within the cap, in whole chunks; every workspace formula covers what its launch writes"""
    for B in (1, 2, 3, 5, 9, 16, 17, 19, 25, 64, 70, 129, 256):
        for Cin, Cout in ((1, 1), (5, 7), (64, 64), (67, 33), (130, 129), (260, 260), (520, 520), (2048, 1024), (4100, 8200)):
            for HW in (1, 16, 25, 49, 54, 324, 1024):
                N = B * HW
                w = gp.c1_wgrad(N, HW, Cin, Cout)
                assert w["splits"] * w["klen"] >= N and (w["splits"] - 1) * w["klen"] < N, (B, Cin, Cout, HW, w)
                assert 1 <= w["splits"] <= w["want"] <= w["cap"] <= gp.C1_MAX_SPLITS and w["klen"] % 32 == 0
                assert w["written"] <= w["ws_floats"]
                assert (w["cap"] == 1) == (w["in_tiles"] * w["out_tiles"] > 512)
            k = gp.k5_wgrad(B, Cin, Cout, 9, 18)
            assert k["written"] <= k["ws_floats"] and k["splits"] == min(B, 64) and k["max_images"] == math.ceil(B / k["splits"])
        for G, Cg, Og in ((1, 5, 7), (2, 11, 19), (3, 3, 5), (32, 16, 16)):
            m = gp.gc_launch(B, G * Cg, G * Og, G, 18, 17, False)
            assert m["used"] <= m["splits"] <= gp.GC_MAX_SPLITS and m["used"] * m["per"] >= B and (m["used"] - 1) * m["per"] < B and 1 <= m["last_images"] <= m["per"]
            assert m["written"] <= m["ws_floats"]
        for ns, C, HW in ((2, 2, 840 * 840), (3, 6, 437), (3, 6, 4160), (32, 512, 1), (6, 6, 35)):
            m = gp.pm_launch(B, C, HW, ns)
            assert 1 <= m["parts"] <= gp.PM_PARTS and m["written"] <= m["ws_doubles"] and 1 <= m["blocks"] <= gp.PM_MAX_BLOCKS
            assert m["parts"] * 1024 >= min(m["total"], gp.PM_PARTS * 1024)


# ---------------------------------------------------------------- inputs, references
def _macs(c):
    """multiply-adds of one of the case's three operations"""
    k = {"c1": 1, "k5": 25, "gc": 9, "gl": 1, "pm": 0}[c.kind]
    return c.B * c.H * c.W * c.Cout * (c.Cin // c.G) * k


def test_reference_cost_stays_small():
    worst = max(gp.CASES, key=_macs)
    print({c.name: f"{_macs(c) / 1e9:.3f} G" for c in gp.CASES})
    assert worst.name in ("c1_wgrad_four_chunks_scalar", "k5_wgrad_strided") and _macs(worst) <= 0.4e9
    assert max(int(np.prod(c.in_shape)) for c in gp.CASES) <= 3 * 2 * 840 * 840


@pytest.mark.parametrize("name", [c.name for c in gp.CASES])
def test_zero_exclusions_and_conditioned_inputs(name):
    """every element of every tensor has a finite bound (a zero bound only for the exact copies of a PReLU's positive side); PReLU inputs keep
    0.05 from the kink, slopes are distinct"""
    c, d, ref = gp.BY_NAME[name], gp.inputs(name), gp.reference(name)
    shapes = {"out": c.out_shape, "gin": c.in_shape}
    assert set(ref) == ({"out", "gin", "gslope"} if c.kind == "pm" else {"out", "gin", "gw", "gb"})
    for k, (r, bound, A) in ref.items():
        assert r.shape == bound.shape == A.shape and np.all(np.isfinite(r)) and np.all(np.isfinite(bound)) and np.all(bound >= 0)
        if k in shapes:
            assert r.size == int(np.prod(shapes[k]))
        if c.kind == "pm" and k in ("out", "gin"):
            assert np.array_equal(bound > 0, (d["x"] <= 0) & (r != 0))
        else:
            assert np.all(bound > 0), f"{name} {k}: an element without a bound"
    if c.kind == "pm":
        assert float(np.abs(d["x"]).min()) >= 0.05 and len(set(d["slopes"].tolist())) == c.G
        assert float(d["slopes"].min()) >= 0.1 and float(d["slopes"].max()) <= 0.4
        assert ref["gslope"][0].shape == (c.G,)
    else:
        assert ref["gw"][0].size == c.n_weights and ref["gb"][0].size == c.Cout


# ---------------------------------------------------------------- the constants and the teeth of the bound
@functools.lru_cache(maxsize=None)
def _emulated(name):
    return gp.emulate(name)


def test_constants_are_twice_the_measured():
    """largest err / (U A) of the float32 emulations over every case and tensor of each family; c = twice that, rounded up"""
    worst = {}
    for c in gp.CASES:
        if c.kind == "pm":
            continue
        ref = gp.reference(c.name)
        for k, v in _emulated(c.name).items():
            r, _, A = ref[k]
            q = float((np.abs(v.astype(np.float64).reshape(r.shape) - r) / (gp.U * A)).max())
            fam = gp.FAMILY[(c.kind, k)]
            if q > worst.get(fam, (0.0, ""))[0]:
                worst[fam] = (q, f"{c.name} {k}")
    print({f: f"{q:.2f} ({w})" for f, (q, w) in worst.items()})
    assert set(worst) == set(gp.MEASURED_C)
    for fam, (q, _) in worst.items():
        assert abs(q - gp.MEASURED_C[fam]) <= 0.02 * gp.MEASURED_C[fam], (fam, q, gp.MEASURED_C[fam])
        assert gp.C_FAMILY[fam] == math.ceil(2 * gp.MEASURED_C[fam]), (fam, gp.C_FAMILY[fam])
    assert gp.C_FAMILY["direct"] == gp.cp.C_MODE["f32"]


def _worst(name, em, keys=None):
    ref = gp.reference(name)
    return {k: float(gp.ratio(v, ref[k][0], ref[k][1]).max()) for k, v in em.items() if keys is None or k in keys}


@pytest.mark.parametrize("name", ["c1_scalar_chunks", "c1_wgrad_two_chunks", "gl_ragged", "gc_ragged", "pm_parts", "k5_wgrad_strided"])
def test_bound_accepts_the_emulation_in_kernel_order(name):
    r = _worst(name, _emulated(name))
    print(name, {k: round(v, 3) for k, v in r.items()})
    assert all(v <= 1.0 for v in r.values()), r


# case, degradation, the tensors it must push out of the bound
DEGRADED = [
    ("c1_scalar_chunks", "drop_last_k", ("out",)),             # the odd-K tail (k = 66) missing
    ("c1_wgrad_two_chunks", "drop_last_split", ("gw",)),       # the 20-pixel last split missing
    ("gc_ragged", "drop_last_split", ("gw",)),                 # the one-image last split missing
    ("gc_ragged", "drop_last_k", ("out",)),
    ("gl_ragged", "drop_last_k", ("out",)),                    # k = 36, the last of the 5-wide tail chunk
    ("k5_wgrad_strided", "drop_second_image", ("gw",)),        # images 64 .. 69 missing
    ("c1_scalar_chunks", "bf16", ("out", "gin", "gw")),
    ("gl_ragged", "bf16", ("out", "gin", "gw")),
    ("gc_ragged", "bf16", ("out", "gin", "gw")),
    ("pm_parts", "bf16", ("out", "gin", "gslope")),
    ("pm_parts", "parts_layout", ("gslope",)),                 # partials summed [part][slope] instead of [slope][part]
]


@pytest.mark.parametrize("name,degrade,keys", DEGRADED, ids=[f"{n}-{d}" for n, d, _ in DEGRADED])
def test_bound_rejects_degraded_arithmetic(name, degrade, keys):
    r = _worst(name, gp.emulate(name, degrade), keys)
    print(name, degrade, {k: f"x{v:.3g}" for k, v in r.items()})
    assert set(r) == set(keys)
    for k, v in r.items():
        assert v > 1.0, f"{name}: the bound accepts {degrade} in {k} (max err / bound {v:.3f})"
