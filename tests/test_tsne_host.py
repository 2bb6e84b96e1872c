"""not-gpu: the numpy restatement of csrc/tsne.hip's arithmetic (tests/tsne_paths.py) against float64 (tests/tsne_oracle.py) within the bounds
tsne_paths derives, on shapes tests/test_gpu_tsne.py runs on the device; mutations of the gradient that must miss the bound by orders of
magnitude; the one-pass distance formula missing the affinity bound far from the origin; the update and cell restatements on hand-written cases;
apply_r's --map options; the header's, the bindings' and the Lua cdef's new symbols."""
import os
import re

import numpy as np
import pytest

import tsne_oracle as to
import tsne_paths as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(err).all() and np.isfinite(bound).all()
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ------------------------------------------------------------------ affinities: the definition behaves as the issue says
@pytest.mark.parametrize("n,d", [(4, 3), (63, 1), (65, 32), (257, 100)])
def test_the_search_stays_clear_of_the_cap_and_meets_the_tolerance(n, d):
    x = to.gaussian(n, d)
    perplexity = min(30.0, (n - 1) / 3)
    D = to.distances(x)
    P, betas, tries = to.joint(x, perplexity)
    assert tries.max() < to.MAX_TRIES
    assert max(abs(to.row_entropy(D, i, betas[i]) - np.log(perplexity)) for i in range(n)) <= to.TOL
    assert np.array_equal(P, P.T) and not np.diag(P).any() and (P >= 0).all() and abs(P.sum() - 1) <= tp.total_bound(n)
    bound = tp.joint_bound(D, d, betas, P)
    assert np.isfinite(bound).all() and (bound[P > 0] > 0).all() and not np.diag(bound - tp.TINY).any()


def test_far_from_the_origin_the_one_pass_distances_miss_the_affinity_bound():
    x = to.far_from_origin(65, 8)
    D = to.distances(x)
    P, betas, _ = to.joint(x, 20.0)
    bound = tp.joint_bound(D, 8, betas, P)
    restated = to.joint_from_distances(to.distances(x.astype(np.float64)), 20.0)[0]      # the differences: exact in float64
    assert worst(np.abs(restated - P), bound) <= 1
    miss = worst(np.abs(to.joint_from_distances(to.one_pass_distances_f32(x), 20.0)[0] - P), bound)
    print(f"one-pass float32 distances: P err / bound {miss:.3g}")
    assert miss > 100                                                    # orders of magnitude: the case bites


# ------------------------------------------------------------------ gradient and KL
@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("exaggeration", [1.0, 12.0])
def test_restated_gradient_and_kl_meet_their_bounds_and_mutations_miss_them(scale, exaggeration):
    n = 257
    P, y = to.random_joint(n), to.layout(n, scale)
    ref, z = to.gradient(P, y, exaggeration)
    bound = tp.gradient_bound(P, y, exaggeration)
    got, z32 = tp.gradient(P, y, exaggeration)
    ratio = worst(np.abs(got - ref), bound)
    print(f"scale {scale:g} e {exaggeration:g}: gradient err / bound {ratio:.3g}, Z rel err {abs(z32 - z) / z:.3g}")
    assert ratio <= 1 and abs(z32 - z) <= tp.EW * z
    # (at scale 1e-4 every w rounds to 1 - 1e-8: w and w^2 are the same number there, and an exaggeration of 1 is no factor)
    for drop in ("4",) + (("w2",) if scale >= 1 else ()) + (("exaggeration",) if exaggeration != 1 else ()):
        miss = worst(np.abs(tp.gradient(P, y, exaggeration, drop=drop)[0] - ref), bound)
        print(f"  without {drop}: err / bound {miss:.3g}")
        assert miss > 1e3
    dx, dy, w = tp.weights32(y)
    P64 = P.astype(np.float64)
    on = P64 > 0
    kl32 = (P64[on] * (np.log(P64[on]) - np.log(w[on]))).sum() + np.log(z32) * P64.sum()
    assert abs(kl32 - to.kl(P, y)) <= tp.kl_bound(P, y)


# ------------------------------------------------------------------ update and cells by hand
def test_update_by_hand():
    f = np.float32
    y = np.array([[1, 2], [3, 4], [-4, -6], [0, 0]], f)
    grad = np.array([[1, -1], [0.0, -0.0], [2, 2], [-1, 1]], f)
    inc = np.array([[1, 1], [0.0, 5], [-0.0, -1], [-1, 0.0]], f)
    gains = np.array([[1, 1], [1, 1], [0.0125, 1], [1, 0.01]], f)
    ny, ninc, ngains, moved = tp.update(y, grad, inc, gains, eta=10.0, momentum=0.5, min_gain=0.01)
    # signs: (+,+) same, (-,+) differ; (0,0) same, (-0,+) differ; (+,-0) differ, (+,-) differ; (-,-) same, (+,0) differ
    want_gains = np.array([[f(1) * f(0.8), f(1) + f(0.2)], [f(1) * f(0.8), f(1) + f(0.2)], [f(0.0125) + f(0.2), f(1) + f(0.2)], [f(1) * f(0.8), f(0.01) + f(0.2)]], f)
    assert np.array_equal(ngains, want_gains)
    assert np.array_equal(ninc, (f(0.5) * inc - (f(10) * want_gains) * grad).astype(f))
    assert np.array_equal(moved, y + ninc)
    assert np.array_equal(ny, (moved.astype(np.float64) - moved.astype(np.float64).sum(axis=0) / 4).astype(f))
    floor = tp.update(y, grad, grad, np.full((4, 2), 0.0124, f), 10.0, 0.5, 0.01)[2]     # 0.0124 * 0.8 is below the floor
    assert np.array_equal(floor[[0, 2, 3]], np.full((3, 2), 0.01, f)) and floor[1, 0] == f(0.01)
    big = to.layout(1100, 3.0)
    out = tp.update(big, to.layout(1100, 1.0, 1), to.layout(1100, 1.0, 2), np.ones((1100, 2), f), 50.0, 0.8, 0.01)
    assert worst(np.abs(out[0].astype(np.float64).mean(axis=0)), tp.mean_bound(out[3], out[0])) <= 1


def test_cells_by_hand():
    y = np.array([[0, 0], [4, 4], [1, 1], [3, 1], [2, 2], [1, 3], [0.9, 0.9]], np.float32)
    rows, counts = tp.cells(y, 2, 2)
    # the box is [0, 4]^2; (2, 2) is on both borders and goes to the upper cell; (4, 4) is on the box edge and is clamped into it
    assert counts.tolist() == [[3, 1], [1, 2]]
    assert rows.tolist() == [[2, 3], [5, 1]]                              # (1, 1) is the centre of cell (0, 0); (4, 4) and (2, 2) are equally far from (3, 3): the lower row
    rows1, counts1 = tp.cells(y, 1, 1)
    assert rows1.tolist() == [[4]] and counts1.tolist() == [[7]]
    flat = np.array([[5, 1], [5, 2], [5, 3]], np.float32)                 # a degenerate axis: everything in its cell 0; 2 is on the border, and
    rows, counts = tp.cells(flat, 2, 4)                                   # 2 and 3 are equally far from the upper cell's centre 2.5
    assert counts.tolist() == [[1, 0, 0, 0], [2, 0, 0, 0]] and rows.tolist() == [[0, -1, -1, -1], [1, -1, -1, -1]]
    rows32, counts32 = tp.cells(y, 32, 32)                                # fewer rows than cells: every row has its own, the others are empty
    assert sorted(rows32[rows32 >= 0].tolist()) == list(range(7)) and (rows32 == -1).sum() == 32 * 32 - 7 and counts32.sum() == 7


def test_purity_and_blobs():
    x, labels = to.blobs(64, 3, 4)
    assert x.dtype == np.float32 and sorted(set(labels)) == [0, 1, 2, 3]
    y = np.stack([labels * 10.0 + 0.01 * np.arange(64), np.zeros(64)], axis=1)
    assert to.purity(y, labels, 1) == 1.0 and to.purity(y, labels, 10) == 1.0
    assert to.purity(np.stack([np.arange(64.0), np.zeros(64)], axis=1), labels, 1) == 0.0


# ------------------------------------------------------------------ the script's options
def test_apply_r_map_options(capsys):
    from ganrev import apply_r
    base = ["--synthetic", "1x32x32x32"]
    plain = apply_r.parse(base)
    assert apply_r.mapOptions(plain) is None
    for name in ("map", "mapRows", "mapPerplexity", "mapIterations", "mapGrid"):
        assert not hasattr(plain, name)                                   # off leaves the namespace as it was
    assert apply_r.mapOptions(apply_r.parse(base + ["--map"])) == (10000, 30.0, 1000, 32)
    assert apply_r.mapOptions(apply_r.parse(base + ["--map", "--nbImages", "520"])) == (520, 30.0, 1000, 32)
    assert apply_r.mapOptions(apply_r.parse(base + ["--map", "--nbImages", "20000", "--mapRows", "16384", "--mapPerplexity", "50", "--mapIterations", "10",
                                                    "--mapGrid", "8"])) == (16384, 50.0, 10, 8)
    for extra, word in ((["--map", "--nbImages", "20000", "--mapRows", "16385"], "at most 16384"), (["--map", "--mapRows", "90"], "(mapRows - 1) / 3"),
                        (["--map", "--mapRows", "100", "--mapPerplexity", "0.5"], "--mapPerplexity"), (["--map", "--nbImages", "50", "--mapRows", "60"], "nbImages"),
                        (["--map", "--mapRows", "3", "--mapPerplexity", "1"], "--mapRows"), (["--mapRows", "100"], "give --map"), (["--map", "--mapGrid", "0"], "--mapGrid"),
                        (["--map", "--mapIterations", "-1"], "--mapIterations")):
        with pytest.raises(SystemExit):
            apply_r.parse(base + extra)
        assert word in capsys.readouterr().err, extra


def test_map_colours():
    from ganrev import render
    cells = np.array([[0, -1], [3, 2]])
    bg = render.map_colours(cells, labels=np.array([13, 0, -1, 2]))
    assert bg.dtype == np.float32 and bg.shape == (4, 3)
    assert np.array_equal(bg, np.float32([render.MAP_PALETTE[1], render.MAP_FIELD, render.MAP_PALETTE[2], render.MAP_FIELD]))      # labels 13, none, 2, -1
    assert np.array_equal(render.map_colours(cells), np.float32([render.MAP_FIELD] * 4))
    assert len(set(render.MAP_PALETTE)) == len(render.MAP_PALETTE) == 12


def test_default_eta():
    from ganrev import tsne as T
    assert T.defaultEta(300) == 50.0 and T.defaultEta(600) == 50.0 and T.defaultEta(10000) == 10000 / 12.0


def test_the_header_and_the_bindings_declare_the_new_symbols():
    from ganrev import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ganrev.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "gan-reverser_amd", "lua", "hipnn.lua")).read()
    names = ("gr_tsne_affinities_dev", "gr_tsne_gradient_dev", "gr_tsne_update_dev", "gr_tsne_kl_dev", "gr_tsne_run_dev", "gr_map_cells_dev")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in L.EXPORTED_SYMBOLS and name + "(" in lua
        assert hasattr(L.Context, name[3:])
    assert re.search(r"#define GR_TSNE_MAX_N (\d+)", hdr).group(1) == str(tp.MAX_N) == str(L.Context.TSNE_MAX_N)
    src = open(os.path.join(ROOT, "gan-reverser_amd", "csrc", "tsne.hip")).read()
    shared = open(os.path.join(ROOT, "gan-reverser_amd", "csrc", "kernels.h")).read()         # ROWS_PER_BLOCK: the one constant of every family
    for text, name, value in ((shared, "ROWS_PER_BLOCK", tp.RPB), (src, "TS_MAX_TRIES", to.MAX_TRIES)):
        assert re.search(r"constexpr int " + name + r" = (\d+)", text).group(1) == str(value)     # the restatements keep the library's constants
    assert "TS_TOL = 1e-5" in src and to.TOL == 1e-5
    fields = [f for f, _ in L.TsneConfig._fields_]
    struct = re.search(r"typedef struct \{([^}]*)\}\s*gr_tsne_config", hdr).group(1)
    assert fields == re.findall(r"\b(exaggeration|stop_lying_iter|momentum0|momentum1|mom_switch_iter|eta|min_gain)\b", struct)
    make = open(os.path.join(ROOT, "gan-reverser_amd", "csrc", "Makefile")).read()
    assert "build/tsne.o" in make and "EXTRA_tsne = -ffp-contract=off" in make
