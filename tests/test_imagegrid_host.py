"""not-gpu: the numpy twin of the image-grid kernels against hand-written expectations, ganrev.png's writer and reader, and the
--render options of the two scripts."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import imagegrid_oracle as io_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def table(n, c=1, h=2, w=2):
    """image k holds the values k + 0.1, k + 0.2, ... in scan order (channel-major)"""
    base = (np.arange(1, c * h * w + 1, dtype=F) / F(10)).reshape(c, h, w)
    return np.stack([base + F(k) for k in range(n)]).astype(F)


def test_two_by_two_grid_of_two_by_two_images():
    x = table(4)
    g = io_.image_grid([x], [0, 1, 2, 3], 2, lo=0.0, hi=4.0)
    assert g.shape == (1, 4, 4)
    want = np.block([[x[0, 0], x[1, 0]], [x[2, 0], x[3, 0]]]) / F(4)
    assert np.array_equal(g[0], want)


def test_partly_filled_last_row_takes_fill():
    x = table(3)
    g = io_.image_grid([x], [0, 1, 2], 2, fill=0.75, lo=0.0, hi=4.0)
    assert g.shape == (1, 4, 4)
    assert np.array_equal(g[0, 2:, 2:], np.full((2, 2), F(0.75)))
    assert np.array_equal(g[0, 2:, :2], x[2, 0] / F(4))
    # nrow larger than the number of tiles: one row of n_tiles
    assert io_.image_grid([x], [0, 1, 2], 6, lo=0.0, hi=4.0).shape == (1, 2, 6)


def test_padding_two_puts_the_tile_one_pixel_into_its_cell():
    x = table(2)
    g = io_.image_grid([x], [0, 1], 2, padding=2, fill=0.5, lo=0.0, hi=2.0)
    assert g.shape == (1, 4, 8)
    want = np.full((4, 8), F(0.5))
    want[1:3, 1:3] = x[0, 0] / F(2)
    want[1:3, 5:7] = x[1, 0] / F(2)
    assert np.array_equal(g[0], want)


def test_margin_one_with_a_red_tile():
    x = np.full((2, 3, 2, 2), F(0.25))
    g = io_.image_grid([x], [0, 1], 2, from_space=0, margin=1, bg=[[1, 0, 0], [0, 0, 0]])
    assert g.shape == (3, 4, 8)
    red = np.zeros((3, 4, 4), F); red[0] = 1; red[:, 1:3, 1:3] = 0.25
    black = np.zeros((3, 4, 4), F); black[:, 1:3, 1:3] = 0.25
    assert np.array_equal(g[:, :, :4], red) and np.array_equal(g[:, :, 4:], black)


def test_inset_frame_overwrites_the_outer_ring_of_the_image():
    x = np.full((2, 3, 3, 3), F(0.5))
    g = io_.image_grid([x], [0, 1], 2, from_space=0, inset=[1, 0], inset_rgb=(0, 0, 1))
    framed = np.zeros((3, 3, 3), F); framed[2] = 1; framed[:, 1, 1] = 0.5
    assert np.array_equal(g[:, :, :3], framed)
    assert np.array_equal(g[:, :, 3:], np.full((3, 3, 3), F(0.5)))


def test_two_slots_sit_side_by_side_and_a_missing_row_leaves_the_background():
    a, b = table(2), table(2) + F(10)
    g = io_.image_grid([a, b], [[0, 1], [1, -1]], 1, bg=[[0, 0, 0], [20, 0, 0]], lo=0.0, hi=20.0)
    assert g.shape == (1, 4, 4)
    assert np.array_equal(g[0, :2, :2], a[0, 0] / F(20)) and np.array_equal(g[0, :2, 2:], b[1, 0] / F(20))
    assert np.array_equal(g[0, 2:, :2], a[1, 0] / F(20)) and np.array_equal(g[0, 2:, 2:], np.ones((2, 2), F))
    # the blue field of fixed_pairs: (H + 2) x (2 W + 2)
    assert io_.image_grid([np.zeros((1, 3, 5, 4), F)] * 2, [[0, 0]], 4, from_space=0, margin=1).shape == (3, 7, 10)


def test_auto_range_spans_the_tiles_not_the_fill():
    x = np.array([[[[2, 4], [6, 10]]]], F)
    g = io_.image_grid([x], [0, 0, 0], 2, fill=7.0, auto_range=True)
    assert np.array_equal(g[0, :2, :2], np.array([[0, 0.25], [0.5, 1]], F))
    assert np.array_equal(g[0, 2:, 2:], np.full((2, 2), F(7)))
    # a fixed range clamps first
    g = io_.image_grid([x], [0], 1, lo=4.0, hi=8.0)
    assert np.array_equal(g[0], np.array([[0, 0], [0.5, 1]], F))


def test_equal_bounds_give_zero():
    x = np.full((1, 1, 2, 2), F(3))
    assert np.array_equal(io_.image_grid([x], [0], 1, auto_range=True)[0], np.zeros((2, 2), F))
    assert np.array_equal(io_.image_grid([x], [0], 1, lo=1.0, hi=1.0)[0], np.zeros((2, 2), F))


def test_quantisation_and_mean_twins():
    v = np.array([[[0.0, 1.0, 0.5, 0.25, 1.0 / 255, 0.998, -1.0, 2.0]]], F)
    assert io_.quantise(v)[0, :, 0].tolist() == [0, 255, 128, 64, 1, 254, 0, 255]
    assert io_.quantise(np.zeros((3, 2, 5), F)).shape == (2, 5, 3)
    t = table(5, 3)
    assert np.array_equal(io_.rows_mean(t, [3]), t[3])
    assert np.array_equal(io_.rows_mean(t, []), np.zeros_like(t[0]))
    want = ((np.zeros_like(t[0]) + t[4]) + t[0]) + t[4]
    assert np.array_equal(io_.rows_mean(t, [4, 0, 4]), want / F(3))


# ---------------------------------------------------------------------------------------------------------------------
def pictures():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in ((4, 6, 1), (5, 7, 3), (3, 5, 1), (1, 1, 1), (1, 1, 3), (9, 1, 3))]


@pytest.mark.parametrize("k", range(6))
def test_png_round_trip(tmp_path, k):
    from ganrev import png
    u8 = pictures()[k]
    p = str(tmp_path / "a.png")
    png.write_png(p, u8)
    back = png.read_png(p)
    assert back.dtype == np.uint8 and back.shape == u8.shape and np.array_equal(back, u8)
    if u8.shape[2] == 1:                                          # [H x W] is accepted as gray
        png.write_png(p, u8[:, :, 0])
        assert np.array_equal(png.read_png(p), u8)


def filtered_png(u8, ft):
    """a PNG whose every scanline uses filter type ft (1 Sub, 2 Up, 3 Average, 4 Paeth), written from the specification"""
    h, w, c = u8.shape
    flat = u8.reshape(h, w * c).astype(np.int64)
    raw = bytearray()
    for y in range(h):
        raw.append(ft)
        for i in range(w * c):
            a = flat[y, i - c] if i >= c else 0
            b = flat[y - 1, i] if y else 0
            cc = flat[y - 1, i - c] if (y and i >= c) else 0
            if ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                p = a + b - cc
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
            raw.append(int(flat[y, i] - pred) & 255)
    ch = lambda kind, data: struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    comp = zlib.compress(bytes(raw))
    half = len(comp) // 2                                         # two IDAT chunks: the stream may be split anywhere
    return (b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0))
            + ch(b"IDAT", comp[:half]) + ch(b"IDAT", comp[half:]) + ch(b"IEND", b""))


@pytest.mark.parametrize("ft", [1, 2, 3, 4])
def test_read_png_undoes_every_scanline_filter(tmp_path, ft):
    from ganrev import png
    for u8 in pictures():
        p = str(tmp_path / "f.png")
        open(p, "wb").write(filtered_png(u8, ft))
        assert np.array_equal(png.read_png(p), u8), (ft, u8.shape)


def test_read_png_refuses_what_it_does_not_decode(tmp_path):
    from ganrev import png
    with pytest.raises(ValueError):
        png.decode_png(b"not a png at all")
    data = bytearray(png.encode_png(pictures()[0]))
    data[-20] ^= 1                                                # a flipped bit in the IDAT chunk: CRC
    with pytest.raises(ValueError):
        png.decode_png(bytes(data))
    with pytest.raises(ValueError):
        png.encode_png(np.zeros((2, 2, 2), np.uint8))


def test_an_independent_decoder_reads_the_same_pixels(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ganrev import png
    for u8 in pictures():
        p = str(tmp_path / "p.png")
        png.write_png(p, u8)
        with Image.open(p) as im:
            got = np.asarray(im)
        assert np.array_equal(got.reshape(u8.shape), u8)


# ---------------------------------------------------------------------------------------------------------------------
def test_scripts_accept_render_and_default_it_to_off():
    from ganrev import apply_r, sample
    assert apply_r.parse([]).render is False and apply_r.parse(["--render"]).render is True
    assert sample.parse([]).render is False and sample.parse(["--render"]).render is True


def test_product_package_imports_neither_pil_nor_the_oracle():
    pkg = os.path.join(ROOT, "gan-reverser_amd", "ganrev")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r"^\s*(import|from)\s+(PIL|Image|imagegrid_oracle|colorspace_oracle|oracle)\b", src, flags=re.M), f
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import ganrev.png, ganrev.render, ganrev.apply_r, ganrev.sample; "
            "bad = [m for m in sys.modules if m == 'PIL' or m.startswith('PIL.') or 'oracle' in m]; assert not bad, bad"
            % os.path.join(ROOT, "gan-reverser_amd"))
    subprocess.check_call([sys.executable, "-c", code])


def test_grid_shape_follows_the_reference_formulas():
    from ganrev import _lib as L
    assert L.grid_shape(512, 1, 3, 32, 32, 0, 16) == (3, 32 * 32, 16 * 32)                    # variations: noiseDim x nbSteps
    assert L.grid_shape(52, 2, 3, 32, 32, 0, 4, margin=1) == (3, 13 * 34, 4 * 66)             # fixed_pairs
    assert L.grid_shape(528, 1, 1, 32, 32, -1, 22) == (1, 24 * 32, 22 * 32)                   # fixed_images: floor(sqrt(528)) = 22
    assert L.grid_shape(528, 1, 3, 32, 32, 0, 22, margin=1) == (3, 24 * 34, 22 * 34)          # anomalies
    for n in (1, 5, 72, 528):
        for nrow in (1, 4, 30):
            x, y, th, tw, gh, gw = io_.geometry(n, 2, 7, 9, nrow, 2, 1)
            assert L.grid_shape(n, 2, 3, 7, 9, 2, nrow, 2, 1) == (3, gh, gw)
