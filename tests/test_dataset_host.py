"""not-gpu: the numpy twin of image.scale / the loader's fused path (tests/dataset_oracle.py) against its float64 evaluation and
hand-written answers; ganrev.dataset's path listing, permutation and clamping; ganrev.png's grey / RGB / RGBA round trip.

The bound the fp32 twin is held to is derived, not tuned.  Inputs lie in [0, 1] and every tap weight lies in [0, 1], so every
intermediate value of a pass is at most n (the sum of the weights so far) and the result at most 1.  One fp32 rounding perturbs the value
it rounds by at most 2^-24 of it; carried through the convex combination and the division by n it moves the result by at most 2^-24
(first order).  A pass therefore errs by at most R 2^-24 with R = dataset_oracle.roundings(src_len, dst_len): 0 for a copy, 4 for
up-scaling (1 - f, two products, one sum), and for the box average 1 - f0, its product, one sum into acc and one into n per middle tap,
the last tap's product and two sums, and the division.  The column pass averages row-pass results with weights summing to one, so their
errors add: bound = (R_row + R_col + 1) 2^-24, the + 1 being the byte / 255 division of the fused path.  The indices and weights are the
fp32 ones in both evaluations (they define the filter), so they contribute nothing."""
import os

import numpy as np
import pytest

import dataset_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (sh, sw, dh, dw): both branches in both directions, non-integer ratios, src_len == 1, 48 from 64 ((di + 1) * scale lands on src_len)
PAIRS = [(64, 64, 32, 32), (64, 64, 64, 64), (64, 64, 48, 48), (20, 24, 12, 12), (16, 16, 12, 20), (7, 9, 13, 5), (1, 1, 5, 7),
         (1, 6, 4, 3), (5, 1, 3, 8), (33, 31, 32, 32), (10, 10, 25, 17), (64, 48, 8, 128)]


def bound(sh, sw, dh, dw, extra=0):
    return (do.roundings(sw, dw) + do.roundings(sh, dh) + extra) * 2.0 ** -24


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "x".join(map(str, p)))
def test_the_fp32_twin_is_within_the_derived_bound_of_its_float64_evaluation(pair):
    sh, sw, dh, dw = pair
    x = np.random.default_rng(sum(pair)).random((2, 3, sh, sw), dtype=np.float32)
    got, want = do.scale(x, dh, dw), do.scale(x, dh, dw, np.float64)
    assert got.dtype == np.float32 and want.dtype == np.float64 and got.shape == (2, 3, dh, dw)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{pair}: max |fp32 - fp64| = {err:.3e}, bound {bound(*pair):.3e}")
    assert err <= bound(*pair)
    u8 = np.random.default_rng(7).integers(0, 256, (2, sh, sw, 3), dtype=np.uint8)
    err = float(np.abs(do.dataset_images(u8, dh, dw, "rgb").astype(np.float64) - do.dataset_images(u8, dh, dw, "rgb", dtype=np.float64)).max())
    assert err <= bound(*pair, extra=1)


def test_the_last_span_of_48_from_64_ends_exactly_on_the_source_length():
    t = do.taps(64, 48)
    assert t[-1][3] == 64 and t[-1][4] == 0                    # fp32 48 * (64 / 48) == 64: the tap at i1 is skipped
    assert all(tap[1] < 64 for tap in t)


def test_an_equal_size_is_a_copy():
    x = np.random.default_rng(1).random((2, 3, 9, 11), dtype=np.float32)
    assert np.array_equal(do.scale(x, 9, 11).view(np.uint32), x.view(np.uint32))


def test_64_to_32_is_the_mean_of_each_2x2_block_rows_first():
    x = np.random.default_rng(2).random((2, 1, 64, 64), dtype=np.float32)
    rows = (x[..., 0::2] + x[..., 1::2]) / np.float32(2)
    want = (rows[..., 0::2, :] + rows[..., 1::2, :]) / np.float32(2)
    assert np.array_equal(do.scale(x, 32, 32).view(np.uint32), want.view(np.uint32))


def test_up_scaling_reproduces_the_four_corners():
    x = np.random.default_rng(3).random((1, 3, 7, 5), dtype=np.float32)
    y = do.scale(x, 19, 12)
    for (a, b), (c, d) in (((0, 0), (0, 0)), ((0, -1), (0, -1)), ((-1, 0), (-1, 0)), ((-1, -1), (-1, -1))):
        assert np.array_equal(y[..., a, b], x[..., c, d])


def test_a_constant_image_stays_constant():
    """Copy: always, to the last bit.  Up-scaling computes (1 - f) v + f v: for v a power of two (or 0) both products are exact and
    fl(1 - f) + f lies within 2^-25 of 1, so the sum rounds back to v - to the last bit.  For any other v the two products round, and the
    stated arithmetic does NOT give v back in general (0.7071 comes out one ulp high at one pixel of 23 from 10): such constants are held
    to the derived bound, like the down-scaling branch, where acc / n with fractional weights need not round back either."""
    for v in (0.0, 1.0, 0.5, 0.25, 0.3, 0.7071):
        x = np.full((1, 1, 12, 10), v, np.float32)
        assert np.array_equal(do.scale(x, 12, 10).view(np.uint32), x.view(np.uint32))
        up = do.scale(x, 29, 23)
        if v in (0.0, 1.0, 0.5, 0.25):
            assert np.array_equal(up.view(np.uint32), np.full_like(up, v).view(np.uint32))
        assert float(np.abs(up.astype(np.float64) - np.float64(np.float32(v))).max()) <= bound(12, 10, 29, 23)
        down = do.scale(x, 5, 7)
        assert float(np.abs(down.astype(np.float64) - np.float64(np.float32(v))).max()) <= bound(12, 10, 5, 7)


def test_bytes_become_three_planes():
    u8 = np.arange(2 * 3 * 4 * 4, dtype=np.uint8).reshape(2, 3, 4, 4)
    rgba = do.bytes_to_planar(u8)
    assert rgba.shape == (2, 3, 3, 4) and np.array_equal(rgba[0, 2, 1, 1], np.float32(u8[0, 1, 1, 2]) / np.float32(255))
    grey = do.bytes_to_planar(u8[..., :1])
    assert np.array_equal(grey[:, 0], grey[:, 1]) and np.array_equal(grey[:, 0], grey[:, 2])
    assert np.array_equal(do.normalize(np.array([0, 0.25, 1, 1.5], np.float32)), np.array([-1, -0.5, 1, 1], np.float32))


# --------------------------------------------------------------------------------------------------------------------- ganrev.dataset
@pytest.fixture
def DATASET():
    from ganrev import dataset
    saved = {k: getattr(dataset, k) for k in ("dirs", "fileExtension", "height", "width", "nbChannels", "colorSpace", "paths", "_seed", "_draws")}
    yield dataset
    for k, v in saved.items():
        setattr(dataset, k, v)


def touch(d, *names):
    os.makedirs(d, exist_ok=True)
    for n in names:
        open(os.path.join(d, n), "wb").close()


def test_loadPaths_orders_by_bytes_matches_the_suffix_and_accumulates_directories(tmp_path, DATASET):
    a, b = str(tmp_path / "b_dir"), str(tmp_path / "a_dir")
    touch(a, "b.jpg", "B.jpg", "a10.jpg", "a9.jpg", "notes.txt", "xjpg", "c.jpg.bak")
    touch(b, "z.jpg", "é.jpg")
    DATASET.setDirs([a, b]); DATASET.setFileExtension("jpg")
    got = DATASET.loadPaths()
    want = sorted([os.path.join(a, n) for n in ("b.jpg", "B.jpg", "a10.jpg", "a9.jpg", "xjpg")] + [os.path.join(b, n) for n in ("z.jpg", "é.jpg")],
                  key=os.fsencode)
    assert got == want and DATASET.paths == want               # "xjpg" matches: the reference's pattern is ext .. '$', without a dot
    assert got.index(os.path.join(a, "B.jpg")) < got.index(os.path.join(a, "a10.jpg")) < got.index(os.path.join(a, "a9.jpg"))


def test_loadPaths_raises_the_reference_error_for_an_empty_folder(tmp_path, DATASET):
    from ganrev._lib import GanrevError
    touch(str(tmp_path / "e"), "readme.txt")
    DATASET.setDirs([str(tmp_path / "e")]); DATASET.setFileExtension("png")
    with pytest.raises(GanrevError, match="given directory doesnt contain any files of type: png"):
        DATASET.loadPaths()
    with pytest.raises(GanrevError, match="doesnt contain any files"):
        DATASET.imageIndices(1, 3)                              # loadImages loads the paths first (dataset.lua:104-106)


def test_the_drawn_permutation_is_reproducible_per_seed(tmp_path, DATASET):
    touch(str(tmp_path), *["%03d.png" % i for i in range(40)])
    DATASET.setDirs([str(tmp_path)]); DATASET.setFileExtension("png")
    a, b, c = DATASET.randomIndices(10, seed=5), DATASET.randomIndices(10, seed=5), DATASET.randomIndices(10, seed=6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, np.random.Generator(np.random.PCG64(5)).permutation(40)[:10])
    assert len(set(a.tolist())) == 10 and a.min() >= 0 and a.max() < 40
    assert len(DATASET.randomIndices(1000, seed=1)) == 40      # dataset.lua:143: min(count, #paths)
    DATASET.setSeed(3)
    first, second = DATASET.randomIndices(40), DATASET.randomIndices(40)
    DATASET.setSeed(3)
    assert np.array_equal(first, DATASET.randomIndices(40)) and np.array_equal(second, DATASET.randomIndices(40))
    assert not np.array_equal(first, second)                    # successive epochs draw different images


def test_loadImages_clamps_to_the_files_that_exist(tmp_path, DATASET):
    touch(str(tmp_path), *["%02d.png" % i for i in range(10)])
    DATASET.setDirs([str(tmp_path)]); DATASET.setFileExtension("png")
    assert DATASET.imageIndices(1, 9999999).tolist() == list(range(10))
    assert DATASET.imageIndices(4, 3).tolist() == [3, 4, 5]
    assert DATASET.imageIndices(8, 5).tolist() == [7, 8, 9]    # the reference would take min(5, 10) = 5 and index past the end
    assert DATASET.imageIndices(11, 5).tolist() == []
    with pytest.raises(AssertionError):
        DATASET.imageIndices(0, 5)                              # dataset.lua:100
    with pytest.raises(AssertionError):
        DATASET.imageIndices(1, 0)                              # dataset.lua:101


def test_setters_and_decoders(tmp_path, DATASET):
    from ganrev._lib import GanrevError
    from ganrev import png
    with pytest.raises(AssertionError):
        DATASET.setColorSpace("lab")                            # dataset.lua:28-31
    DATASET.setDirs("one"); assert DATASET.dirs == ["one"]
    rng = np.random.default_rng(4)
    for c in (1, 3, 4):
        u8 = rng.integers(0, 256, (5, 7, c), dtype=np.uint8)
        png.write_png(str(tmp_path / "a.png"), u8)
        assert np.array_equal(DATASET.decode(str(tmp_path / "a.png")), u8)
        np.save(str(tmp_path / "a.npy"), u8)
        assert np.array_equal(DATASET.decode(str(tmp_path / "a.npy")), u8)
    np.save(str(tmp_path / "f.npy"), np.zeros((4, 4, 3), np.float32))
    with pytest.raises(GanrevError, match="uint8"):
        DATASET.decode(str(tmp_path / "f.npy"))


def test_png_round_trips_grey_rgb_and_rgba(tmp_path):
    from ganrev import png
    rng = np.random.default_rng(9)
    for c in (1, 3, 4):
        for h, w in ((1, 1), (5, 9), (32, 31)):
            u8 = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
            p = str(tmp_path / "x.png")
            png.write_png(p, u8)
            back = png.read_png(p)
            assert back.dtype == np.uint8 and back.shape == (h, w, c) and np.array_equal(back, u8)


def test_scripts_take_dataset_and_refuse_it_beside_data():
    from ganrev import apply_r, pretrain_g, pretrain_with_previous_net, sample, scripts, train, train_r
    from ganrev._lib import GanrevError
    for mod in (train, train_r, apply_r, pretrain_g, pretrain_with_previous_net, sample):
        o = mod.parse([])
        assert o.dataset == "NONE" and o.fileExtension == "jpg", mod.__name__
        o = mod.parse(["--dataset", "faces", "--fileExtension", "png"])
        assert o.dataset == "faces" and o.fileExtension == "png"
    o = train.parse(["--dataset", "faces", "--data", "x.npy"])
    with pytest.raises(GanrevError, match="both"):
        scripts.open_dataset(o, "rgb", 32, 32)
    assert scripts.open_dataset(train.parse([]), "rgb", 32, 32) is None


def test_a_checkpoints_opt_names_the_dataset_only_when_one_is_read():
    """--data and the synthetic default keep their behaviour bit for bit, the saved `opt` included: without --dataset the table holds
    exactly the keys it held before the two options existed, in the same order; with it, both are saved in the parser's order."""
    from ganrev import pretrain_g, pretrain_with_previous_net, scripts, train, train_r
    for mod in (train, train_r, pretrain_g, pretrain_with_previous_net):
        o = mod.parse([])
        plain = scripts.opt_table(o)
        assert "dataset" not in plain and "fileExtension" not in plain, mod.__name__
        scalars = [k.rstrip("_") for k, v in vars(o).items() if isinstance(v, (int, float, str, bool))]
        assert list(plain) == [k for k in scalars if k not in ("dataset", "fileExtension")]
        named = scripts.opt_table(mod.parse(["--dataset", "faces", "--fileExtension", "png"]))
        assert named["dataset"] == "faces" and named["fileExtension"] == "png" and list(named) == scalars


def test_header_cdef_and_bindings_name_the_new_entry_points():
    import ganrev._lib as L
    hdr = open(os.path.join(ROOT, "include", "ganrev.h")).read()
    lua = open(os.path.join(ROOT, "gan-reverser_amd", "lua", "hipnn.lua")).read()
    for name in ("gr_image_scale_dev", "gr_image_scale_host", "gr_dataset_images_dev"):
        assert name + "(" in hdr and name + "(" in lua and name in L.EXPORTED_SYMBOLS
