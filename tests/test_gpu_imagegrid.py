"""gpu: gr_image_grid_dev, gr_rows_mean_dev and gr_l2_distance_rows_dev against their numpy twins (tests/imagegrid_oracle.py), bit for
bit - np.array_equal on the uint32 view of the float grid and on the uint8 picture, no tolerance: every operation of these kernels is a
single fp32 operation in a stated order - then ganrev.render's seven products and python -m ganrev.apply_r --render end to end.

The error-path tests hand the library arguments its HOST-side checks refuse: nothing is launched, nothing on the device can fault."""
import json
import math
import os

import numpy as np
import pytest

import colorspace_oracle as co
import imagegrid_oracle as io_

pytestmark = pytest.mark.gpu
F = np.float32


class Tables:
    """device copies of host tables, optionally 4 bytes into their allocation (no 16-byte alignment to lean on); freed on exit"""

    def __init__(self, ctx, arrays, offset=0):
        self.ctx, self.base, self.ptrs = ctx, [], []
        for a in arrays:
            b = ctx.malloc(a.nbytes + offset)
            self.base.append(b)
            self.ptrs.append(b + offset)
            ctx.upload(np.ascontiguousarray(a, F), b + offset)

    def __enter__(self):
        return self.ptrs

    def __exit__(self, *exc):
        for b in self.base:
            self.ctx.free(b)


def run_grid(ctx, arrays, rows, nrow, from_space, offset=0, **kw):
    """-> (float grid [Cout x GH x GW], u8 [GH x GW x Cout]) from the device"""
    _, c, h, w = arrays[0].shape
    rows = np.asarray(rows, np.int64).reshape(-1, len(arrays))
    gh, gw = io_.geometry(len(rows), len(arrays), h, w, nrow, kw.get("padding", 0), kw.get("margin", 0))[4:]
    cout = 3 if from_space >= 0 else c
    with Tables(ctx, arrays, offset) as ptrs:
        gd, ud = ctx.malloc(4 * cout * gh * gw), ctx.malloc(cout * gh * gw)
        try:
            shape = ctx.image_grid_dev(ptrs, [len(a) for a in arrays], c, h, w, from_space, rows, nrow, grid_dev=gd, u8_dev=ud, **kw)
            assert shape == (cout, gh, gw)
            return ctx.download(gd, (cout, gh, gw), F), ctx.download(ud, (gh, gw, cout), np.uint8)
        finally:
            ctx.free(gd); ctx.free(ud)


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad[0]), f"{len(bad[0])} of {got.size} values differ; first at {tuple(int(b[0]) for b in bad)}: {got[bad][0]!r} != {want[bad][0]!r}"


def check(ctx, arrays, rows, nrow, from_space, offset=0, **kw):
    g, u = run_grid(ctx, arrays, rows, nrow, from_space, offset, **kw)
    want = io_.image_grid(arrays, rows, nrow, from_space, **kw)
    same_bits(g, want)
    assert np.array_equal(u, io_.quantise(want))
    return g, u


def images(n, space, h, w, seed):
    return co.make_images((n, h, w), co.SPACES[space] if space >= 0 else "rgb", seed)


@pytest.mark.parametrize("from_space", [0, 1, 2, 3, -1])
@pytest.mark.parametrize("hw", [(32, 32), (64, 64), (7, 9)])
def test_every_colour_space_and_image_size(ctx, from_space, hw):
    h, w = hw
    x = images(40, from_space, h, w, 11 + from_space)
    rng = np.random.default_rng(h)
    rows = rng.integers(0, 40, 23)
    rows[3] = rows[4] = rows[9]                                    # repeated rows
    rows[7] = -1                                                   # an empty tile
    check(ctx, [x], rows, 5, from_space, offset=4 if hw == (7, 9) else 0)


def test_one_channel_table_copied_as_it_is_gives_a_one_channel_grid(ctx):
    x = images(9, 1, 32, 32, 3)
    g, u = check(ctx, [x], np.arange(9), 3, -1, padding=2, fill=0.5)
    assert g.shape == (1, 3 * 34, 3 * 34) and u.shape == (3 * 34, 3 * 34, 1)


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("padding", [0, 2])
@pytest.mark.parametrize("auto", [False, True])
def test_slots_margins_padding_backgrounds_insets_and_both_ranges(ctx, slots, margin, padding, auto):
    n_tiles = 11                                                   # not a multiple of nrow = 4
    tabs = [images(30, 3, 7, 9, 21), images(17, 3, 7, 9, 22)][:slots]
    rng = np.random.default_rng(100 * slots + 10 * margin + padding + auto)
    rows = np.stack([rng.integers(-1, len(t), n_tiles) for t in tabs], axis=1)
    rows[2] = -1
    bg = rng.random((n_tiles, 3)).astype(F)
    bg[0], bg[1], bg[5] = (1, 0, 0), (0, 0, 0), (0, 0, 1)
    inset = (np.arange(n_tiles) % 3 == 0).astype(np.uint8)
    check(ctx, tabs, rows, 4, 3, offset=4, padding=padding, margin=margin, bg=bg, inset=inset, inset_rgb=(0.0, 0.25, 1.0),
          fill=0.875, auto_range=auto, lo=0.125, hi=0.75)


def test_values_outside_a_fixed_range_clamp_and_equal_bounds_give_zero(ctx):
    x = images(6, 0, 32, 32, 8)                                    # holds out-of-gamut values above 1
    check(ctx, [x], np.arange(6), 3, 0, lo=0.25, hi=0.5)
    g, u = check(ctx, [x], np.arange(6), 3, 0, lo=0.5, hi=0.5)
    assert not g.any() and not u.any()
    flat = np.full((2, 3, 7, 9), F(0.3))
    g, _ = check(ctx, [flat], [0, 1], 2, 0, auto_range=True)
    assert not g.any()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def faces(ctx):
    from ganrev.nn_utils import DeviceTensor
    made = []

    def make(n, space, seed, h=32, w=32):
        x = images(n, co.SPACES.index(space), h, w, seed)
        t = DeviceTensor(ctx, x.shape)
        ctx.upload(x, t.ptr)
        made.append(t)
        return x, t
    yield make
    for t in made:
        t.free()


def test_product_variations(ctx, faces, tmp_path):
    from ganrev import png, render
    x, t = faces(48, "rgb", 1)
    u = render.variations_grid(t, 16, path=str(tmp_path / "v.png"))
    want = io_.quantise(io_.image_grid([x], np.arange(48), 16, -1))
    assert np.array_equal(u, want) and np.array_equal(png.read_png(str(tmp_path / "v.png")), want)


def test_product_cluster(ctx, faces):
    from ganrev import render
    x, t = faces(200, "yuv", 2)
    rows = np.random.default_rng(2).permutation(200)[:71]
    face = io_.rows_mean(x, rows)
    want = io_.quantise(io_.image_grid([np.concatenate([face[None], x[rows]])], np.arange(72), math.ceil(math.sqrt(72)), 2))
    assert np.array_equal(render.cluster_grid(t, rows, "yuv"), want)
    assert want.shape == (8 * 32, 9 * 32, 3)                       # 72 tiles, ceil(sqrt(72)) = 9 per row, 8 rows


def test_product_similar(ctx, faces):
    from ganrev import render
    x, t = faces(300, "hsl", 3)
    rows = np.random.default_rng(3).permutation(300)[:100]
    inset = np.zeros(100, np.uint8); inset[0] = 1
    want = io_.quantise(io_.image_grid([x], rows, 10, 3, inset=inset, inset_rgb=(0, 0, 1)))
    u = render.similar_grid(t, rows, "hsl")
    assert np.array_equal(u, want)
    assert (u[0, :32] == (0, 0, 255)).all() and (u[31, :32] == (0, 0, 255)).all() and (u[:32, 0] == (0, 0, 255)).all()


def test_product_fixed_pairs(ctx, faces):
    from ganrev import render
    x, t = faces(60, "rgb", 4)
    y, s = faces(52, "rgb", 5)
    i = np.arange(52)
    want = io_.quantise(io_.image_grid([x, y], np.stack([i, i], 1), 4, 0, margin=1, bg=np.tile(F([0, 0, 1]), (52, 1))))
    u = render.fixed_pairs_grid(t, s, 52, "rgb")
    assert np.array_equal(u, want) and u.shape == (13 * 34, 4 * 66, 3)
    assert (u[0] == (0, 0, 255)).all()


def test_product_fixed_images_skip_the_colour_conversion(ctx, faces):
    from ganrev import render
    x, t = faces(40, "yuv", 6)
    want = io_.quantise(io_.image_grid([x], np.arange(30), 5, -1))
    assert np.array_equal(render.fixed_images_grid(t, 30), want)
    x1, t1 = faces(10, "y", 7)
    u = render.fixed_images_grid(t1, 10)
    assert u.shape == (4 * 32, 3 * 32, 1) and np.array_equal(u, io_.quantise(io_.image_grid([x1], np.arange(10), 3, -1)))


def test_product_anomalies(ctx, faces):
    from ganrev import render
    x, t = faces(64, "y", 8)
    flag = np.random.default_rng(8).random(50) < 0.2
    bg = np.where(flag[:, None], F([1, 0, 0]), F([0, 0, 0])).astype(F)
    want = io_.quantise(io_.image_grid([x], np.arange(50), 7, 1, margin=1, bg=bg))
    u = render.anomalies_grid(t, flag, "y")
    assert np.array_equal(u, want)
    k = int(np.nonzero(flag)[0][0])
    assert tuple(u[(k // 7) * 34, (k % 7) * 34]) == (255, 0, 0)


def test_product_neighbours_takes_its_range_from_the_picture(ctx, faces):
    from ganrev import render
    x, t = faces(20, "rgb", 9)
    y, s = faces(500, "rgb", 10)
    nb = np.random.default_rng(9).integers(0, 500, 16)
    f = io_.image_grid([x, y], np.stack([np.arange(16), nb], 1), 8, 0, auto_range=True)
    assert np.array_equal(render.neighbours_grid(t, np.arange(16), s, nb, "rgb"), io_.quantise(f))
    assert f.shape == (3, 64, 512) and f.min() == 0 and f.max() == 1
    # the layout is toDisplayTensor's over the interleaved list with nrow = the number of pairs
    both = np.empty((32,) + x.shape[1:], F); both[0::2] = x[:16]; both[1::2] = y[nb]
    same_bits(f, io_.image_grid([both], np.arange(32), 16, 0, auto_range=True))
    with pytest.raises(ValueError):
        render.neighbours_grid(t, np.arange(3), s, nb[:3], "rgb")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 71])
def test_rows_mean(ctx, n):
    x = images(300, 0, 32, 32, 30 + n)
    rows = np.random.default_rng(n).integers(0, 300, n)
    with Tables(ctx, [x]) as (p,):
        out = ctx.malloc(4 * 3 * 32 * 32)
        try:
            ctx.upload(np.full(3 * 32 * 32, F(7)), out)           # n == 0 must WRITE zeros
            ctx.rows_mean_dev(p, 300, 3 * 32 * 32, rows, out)
            got = ctx.download(out, (3, 32, 32), F)
        finally:
            ctx.free(out)
    same_bits(got, io_.rows_mean(x, rows))


def test_l2_distance_rows_dev_is_the_host_call_on_resident_tables(ctx):
    a, b = images(130, 0, 32, 32, 40), images(130, 0, 32, 32, 41)
    b[5] = a[5]
    with Tables(ctx, [a, b]) as (pa, pb):
        got = ctx.l2_distance_rows_dev(pa, pb, 130, 3 * 32 * 32)
    want = ctx.l2_distance_rows(a, b)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    d = np.abs(a.reshape(130, -1) - b.reshape(130, -1))
    ref = np.sqrt((d * d).astype(np.float64).sum(axis=1))
    assert got[5] == 0 and np.allclose(got, ref, rtol=1e-12, atol=0)


def kernels_of(ctx, fn):
    ctx.set_timing(2)
    try:
        fn()
        return {k["kernel"]: k["launches"] for k in ctx.kernel_times() if k["kernel"] != "range_guard_fallback"}
    finally:
        ctx.set_timing(0)


def test_launch_counts(ctx):
    x = images(12, 0, 32, 32, 50)
    assert kernels_of(ctx, lambda: run_grid(ctx, [x], np.arange(12), 4, 0)) == {"image_grid_kernel": 1}
    assert kernels_of(ctx, lambda: run_grid(ctx, [x], np.arange(12), 4, 3, auto_range=True)) == {"image_grid_range_kernel": 1, "image_grid_kernel": 1}
    with Tables(ctx, [x]) as (p,):
        out = ctx.malloc(4 * 3 * 32 * 32)
        try:
            assert kernels_of(ctx, lambda: ctx.rows_mean_dev(p, 12, 3 * 32 * 32, [1, 2, 3], out)) == {"rows_mean_kernel": 1}
            assert kernels_of(ctx, lambda: ctx.l2_distance_rows_dev(p, p, 12, 3 * 32 * 32)) == {"l2_distance_rows_kernel": 1}
        finally:
            ctx.free(out)


def test_bad_arguments_are_refused_on_the_host_and_leave_nothing_behind(ctx):
    """argument checks only: each call returns GR_ERR_INVALID before anything is uploaded or launched"""
    from ganrev._lib import GanrevError
    x = images(12, 0, 32, 32, 60)
    with Tables(ctx, [x]) as (p,):
        ud = ctx.malloc(3 * 64 * 64)
        try:
            good = lambda **kw: ctx.image_grid_dev([p], [12], 3, 32, 32, 0, kw.pop("rows", [0, 1, 2, 3]), 2, u8_dev=kw.pop("u8_dev", ud), **kw)

            def refused(fn, word):
                ctx.set_timing(2)
                try:
                    with pytest.raises(GanrevError, match=word):
                        fn()
                    assert [k for k in ctx.kernel_times() if k["kernel"] != "range_guard_fallback"] == []      # nothing was launched
                finally:
                    ctx.set_timing(0)
                assert good() == (3, 64, 64)                       # no sticky state: the next valid call succeeds
            refused(lambda: good(rows=[0, 1, 12, 3]), "GR_ERR_INVALID.*row 12")
            refused(lambda: good(rows=[0, -2, 1, 3]), "GR_ERR_INVALID.*row -2")
            refused(lambda: ctx.image_grid_dev([p, p, p], [12, 12, 12], 3, 32, 32, 0, np.zeros((4, 3), np.int64), 2, u8_dev=ud), "GR_ERR_INVALID.*slots 3")
            refused(lambda: good(u8_dev=None), "GR_ERR_INVALID.*both outputs")
            refused(lambda: good(margin=2), "GR_ERR_INVALID.*geometry")
            refused(lambda: ctx.image_grid_dev([p], [12], 3, 32, 32, 1, [0], 1, u8_dev=ud), "GR_ERR_INVALID.*channel")
            refused(lambda: good(lo=1.0, hi=0.0), "GR_ERR_INVALID.*range")
            refused(lambda: ctx.rows_mean_dev(p, 12, 3 * 32 * 32, [0, 12], ud), "GR_ERR_INVALID.*rows\\[1\\]")
            want = io_.quantise(io_.image_grid([x], [0, 1, 2, 3], 2, 0))
            good()
            assert np.array_equal(ctx.download(ud, (64, 64, 3), np.uint8), want)
        finally:
            ctx.free(ud)


# ---------------------------------------------------------------------------------------------------------------------
def test_apply_r_render_end_to_end(ctx, tmp_path, monkeypatch):
    from ganrev import apply_r, png
    seen = {}
    inner = apply_r.renderAnalysis

    def spy(OPT, out, colorSpace, MODEL_G, images, *rest):
        seen["images"], seen["space"] = images.numpy(), colorSpace
        return inner(OPT, out, colorSpace, MODEL_G, images, *rest)
    monkeypatch.setattr(apply_r, "renderAnalysis", spy)
    a, b = str(tmp_path / "with"), str(tmp_path / "without")
    args = ["--synthetic", "3x32x32x32", "--nbImages", "1200", "--batchSize", "256", "--quiet"]
    s1 = apply_r.main(args + ["--render", "--writeTo", a])
    s0 = apply_r.main(args + ["--writeTo", b])
    assert not [f for f in os.listdir(b) if f.endswith(".png")]
    strip = lambda s: {k: v for k, v in s.items() if "seconds" not in k}
    assert strip(s0) == strip(s1)
    assert strip(json.load(open(os.path.join(a, "summary.json")))) == strip(json.load(open(os.path.join(b, "summary.json"))))
    for name in ("attributes", "similar_by_attributes", "similar_by_pixels", "anomaly_distances", "fixed_faces", "cluster_centroids"):
        assert np.array_equal(np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))), name

    x = seen["images"]
    assert x.shape == (1200, 3, 32, 32) and seen["space"] == "rgb"
    sizes = {"variations.png": (32 * 32, 16 * 32, 3),                       # noiseDim rows of nbSteps
             "fixed_pairs.png": (13 * 34, 4 * 66, 3),                       # 52 pairs, 4 per row, (H + 2) x (2 W + 2)
             "fixed_images_528.png": (24 * 32, 22 * 32, 3), "fixed_images_528_unfixed.png": (24 * 32, 22 * 32, 3),
             "anomalies.png": (24 * 34, 22 * 34, 3)}
    for i in range(1, 6):
        sizes["similar_attributes_%02d.png" % i] = sizes["similar_pixelwise_%02d.png" % i] = (320, 320, 3)
    for j, n in enumerate(s1["cluster_sizes"]):
        if n:
            side = math.ceil(math.sqrt(1 + n))
            sizes["cluster_%02d.png" % (j + 1)] = (-(-(1 + n) // side) * 32, side * 32, 3)
    assert any(s1["cluster_sizes"])
    assert sorted(f for f in os.listdir(a) if f.endswith(".png")) == sorted(sizes)
    for f, shape in sizes.items():
        assert png.read_png(os.path.join(a, f)).shape == shape, f

    rows = np.load(os.path.join(a, "similar_by_attributes.npy"))[0]
    assert len(rows) == 100                       # the frame goes on the first image shown, as apply_r.lua:286-295 frames tnsr[1]
    inset = np.zeros(100, np.uint8); inset[0] = 1
    want = io_.quantise(io_.image_grid([x], rows, 10, 0, inset=inset, inset_rgb=(0, 0, 1)))
    assert np.array_equal(png.read_png(os.path.join(a, "similar_attributes_01.png")), want)

    dist = np.load(os.path.join(a, "anomaly_distances.npy"))
    assert dist.shape == (1024,)
    below = np.sort(dist)[int(math.floor(1024 * 0.15)) - 1]
    flag = (dist <= below)[:528]
    bg = np.where(flag[:, None], F([1, 0, 0]), F([0, 0, 0])).astype(F)
    want = io_.quantise(io_.image_grid([x], np.arange(528), 22, 0, margin=1, bg=bg))
    assert np.array_equal(png.read_png(os.path.join(a, "anomalies.png")), want)
    want = io_.quantise(io_.image_grid([x], np.arange(528), 22, -1))
    assert np.array_equal(png.read_png(os.path.join(a, "fixed_images_528_unfixed.png")), want)
