"""gpu: gr_image_scale_dev / gr_image_scale_host / gr_dataset_images_dev (dataset.lua:111-116,149-153) against the fp32 twin of
tests/dataset_oracle.py, bit for bit; the fused path against the unfused chain of four steps; every error path; ganrev.dataset on a
folder of PNG files of two sizes; and the scripts' --dataset end to end.

"Bit for bit" means np.array_equal on the uint32 views: no tolerance.  It holds because every operation of the kernels is one IEEE fp32
operation in the order the twin states (dataset.hip is compiled with -ffp-contract=off and `/` is the correctly rounded division)."""
import ctypes as C
import os

import numpy as np
import pytest

import colorspace_oracle as co
import dataset_oracle as do
from test_gpu_colorspace import assert_bit_identical, cs, kernels_of

pytestmark = pytest.mark.gpu

# (sh, sw, dh, dw): both branches in both directions, non-integer ratios, src_len == 1, 48 from 64 ((di + 1) * scale == src_len in fp32);
# dw % 4 == 0 selects the 16-byte form, any other dw the scalar one
SCALE_PAIRS = [(64, 64, 32, 32), (64, 64, 64, 64), (64, 64, 48, 48), (20, 24, 12, 12), (16, 16, 12, 20), (7, 9, 13, 5), (1, 1, 5, 7),
               (1, 6, 4, 3), (5, 1, 3, 8), (33, 31, 32, 32), (10, 10, 25, 17), (64, 48, 8, 128), (9, 9, 9, 9), (31, 64, 31, 30)]


def test_the_twin_handles_every_chosen_pair():
    for sh, sw, dh, dw in SCALE_PAIRS:
        assert len(do.taps(sw, dw)) == dw and len(do.taps(sh, dh)) == dh      # taps() asserts every index it yields


def dev_scale(ctx, x, dh, dw, offset_floats=0):
    n, planes, sh, sw = x.shape
    din = ctx.malloc(4 * (x.size + offset_floats))
    dout = ctx.malloc(4 * (n * planes * dh * dw + offset_floats))
    try:
        ctx.upload(x, din + 4 * offset_floats)
        ctx.image_scale_dev(din + 4 * offset_floats, n, planes, sh, sw, dh, dw, dout + 4 * offset_floats)
        return ctx.download(dout + 4 * offset_floats, (n, planes, dh, dw))
    finally:
        ctx.free(din); ctx.free(dout)


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("pair", SCALE_PAIRS, ids=lambda p: "x".join(map(str, p)))
def test_image_scale_is_bit_identical_to_the_twin(ctx, pair, planes):
    sh, sw, dh, dw = pair
    x = np.random.default_rng(sum(pair) + planes).random((3, planes, sh, sw), dtype=np.float32)
    x[0, 0] = 0.3                                                        # a constant plane
    want = do.scale(x, dh, dw)
    got, kt = kernels_of(ctx, lambda: dev_scale(ctx, x, dh, dw))
    assert_bit_identical(got, want, f"gr_image_scale_dev {pair} x{planes}")
    assert [(k["kernel"], k["launches"]) for k in kt] == [("image_scale_kernel_v4" if dw % 4 == 0 else "image_scale_kernel", 1)], kt
    assert_bit_identical(ctx.image_scale(x, dh, dw), want, f"gr_image_scale_host {pair} x{planes}")


def test_image_scale_4_bytes_into_its_allocation_takes_the_scalar_form(ctx):
    x = np.random.default_rng(5).random((2, 3, 24, 20), dtype=np.float32)
    for dh, dw in ((12, 12), (24, 20), (40, 32)):
        got, kt = kernels_of(ctx, lambda: dev_scale(ctx, x, dh, dw, offset_floats=1))
        assert_bit_identical(got, do.scale(x, dh, dw), f"at +4 bytes -> {dh} x {dw}")
        assert [(k["kernel"], k["launches"]) for k in kt] == [("image_scale_kernel", 1)], kt


def make_bytes(shape, seed):
    """uint8 [n x sh x sw x sc]: uniform bytes with a block of exact greys, 0 / 255 corners and two-way ties (the hsl branches)"""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, shape, dtype=np.uint8)
    flat = u8.reshape(-1, shape[3])
    k = max(1, flat.shape[0] // 8)
    if shape[3] >= 3:
        flat[0:k, 1] = flat[0:k, 0]; flat[0:k, 2] = flat[0:k, 0]
        flat[k:2 * k, :3] = rng.integers(0, 2, (k, 3), dtype=np.uint8) * 255
        flat[2 * k:3 * k, 1] = flat[2 * k:3 * k, 0]
        flat[3 * k:4 * k, 2] = flat[3 * k:4 * k, 1]
    return u8


def dev_dataset(ctx, u8, dh, dw, to, normalise, offset_bytes=0, offset_floats=0):
    n, sh, sw, sc = u8.shape
    nout = n * co.PLANES[to] * dh * dw
    din = ctx.malloc(u8.size + offset_bytes + 16)
    dout = ctx.malloc(4 * (nout + offset_floats))
    try:
        ctx.upload(u8, din + offset_bytes)
        ctx.dataset_images_dev(din + offset_bytes, n, sh, sw, sc, dh, dw, cs(to), normalise, dout + 4 * offset_floats)
        return ctx.download(dout + 4 * offset_floats, (n, co.PLANES[to], dh, dw))
    finally:
        ctx.free(din); ctx.free(dout)


def unfused_chain(ctx, u8, dh, dw, to, normalise):
    """bytes -> / 255 planar (host), gr_image_scale_dev, gr_colorspace_dev(rgb -> to), normalise (host)"""
    planar = do.bytes_to_planar(u8)
    n = len(planar)
    scaled = dev_scale(ctx, planar, dh, dw)
    d = ctx.upload(scaled)
    dout = ctx.malloc(4 * n * co.PLANES[to] * dh * dw)
    try:
        ctx.colorspace_dev(d, cs("rgb"), cs(to), n, dh, dw, dout)
        out = ctx.download(dout, (n, co.PLANES[to], dh, dw))
    finally:
        ctx.free(d); ctx.free(dout)
    return do.normalize(out) if normalise else out


DATASET_SHAPES = [((5, 64, 64), (32, 32)), ((3, 20, 24), (12, 12)), ((4, 9, 7), (9, 7)), ((3, 10, 10), (25, 17)), ((2, 16, 12), (24, 32)),
                  ((3, 64, 64), (48, 48)), ((1, 5, 3), (4, 8))]        # the last: 5 * 3 * 3 bytes do not end on a dword: scalar form for sc 3


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("to", co.SPACES)
@pytest.mark.parametrize("sc", [1, 3, 4])
def test_dataset_images_is_bit_identical_to_the_twin_and_to_the_unfused_chain(ctx, sc, to, normalise):
    for (n, sh, sw), (dh, dw) in DATASET_SHAPES:
        u8 = make_bytes((n, sh, sw, sc), 100 * sc + cs(to) + sh)
        want = do.dataset_images(u8, dh, dw, to, normalise)
        what = f"gr_dataset_images_dev sc {sc} -> {to}, {sh} x {sw} -> {dh} x {dw}, normalise {normalise}"
        got, kt = kernels_of(ctx, lambda: dev_dataset(ctx, u8, dh, dw, to, normalise))
        assert_bit_identical(got, want, what)
        v4 = dw % 4 == 0 and u8.size % 4 == 0
        assert [(k["kernel"], k["launches"]) for k in kt] == [("dataset_images_kernel_v4" if v4 else "dataset_images_kernel", 1)], (what, kt)
        assert kt[0]["bytes"] == u8.size + 4 * got.size
        assert_bit_identical(got, unfused_chain(ctx, u8, dh, dw, to, normalise), what + " against the unfused chain")


@pytest.mark.parametrize("sc", [1, 3, 4])
def test_dataset_images_on_misaligned_buffers_takes_the_scalar_form(ctx, sc):
    u8 = make_bytes((3, 16, 16, sc), 40 + sc)
    for ob, of in ((1, 0), (2, 0), (0, 1), (3, 1)):
        got, kt = kernels_of(ctx, lambda: dev_dataset(ctx, u8, 8, 8, "hsl", True, offset_bytes=ob, offset_floats=of))
        assert_bit_identical(got, do.dataset_images(u8, 8, 8, "hsl", True), f"sc {sc} at +{ob} bytes in, +{4 * of} bytes out")
        assert [(k["kernel"], k["launches"]) for k in kt] == [("dataset_images_kernel", 1)], kt


def test_bad_arguments_return_an_error_and_leave_out_untouched(ctx):
    import ganrev._lib as L
    x = np.random.default_rng(1).random((2, 3, 4, 4), dtype=np.float32)
    u8 = make_bytes((2, 4, 4, 3), 1)
    sentinel = np.full(2 * 3 * 8 * 8, 7.25, np.float32)
    din, dbytes, dout = ctx.upload(x), ctx.upload(u8), ctx.upload(sentinel)
    hout = sentinel.copy()
    p = lambda a: None if a is None else (C.c_void_p(a) if isinstance(a, int) else C.c_void_p(a.ctypes.data))
    err = lambda: ctx.lib.gr_last_error(ctx.h).decode()
    try:
        scale_cases = [  # (in, n, planes, sh, sw, dh, dw, out), message
            ((None, 2, 3, 4, 4, 8, 8, dout), "null"), ((din, 2, 3, 4, 4, 8, 8, None), "null"),
            ((din, 0, 3, 4, 4, 8, 8, dout), "positive"), ((din, 2, 0, 4, 4, 8, 8, dout), "positive"), ((din, 2, 3, 0, 4, 8, 8, dout), "positive"),
            ((din, 2, 3, 4, -1, 8, 8, dout), "positive"), ((din, 2, 3, 4, 4, 0, 8, dout), "positive"), ((din, 2, 3, 4, 4, 8, 0, dout), "positive"),
            ((din, 2, 3, 4, 4, 8, 40000, dout), "too large"), ((din, 2, 3, 4, 40000, 8, 8, dout), "too large"),
            ((din, 1 << 40, 3, 4, 4, 8, 8, dout), "too large a batch"), ((dout, 2, 3, 4, 4, 8, 8, dout), "in place"),
        ]
        for (a_in, n, pl, sh, sw, dh, dw, a_out), msg in scale_cases:
            rc = ctx.lib.gr_image_scale_dev(ctx.h, p(a_in), n, pl, sh, sw, dh, dw, p(a_out))
            assert rc == -1 and msg in err(), (rc, msg, err())
            hin = None if a_in is None else (hout if a_in == dout else x)
            rc = ctx.lib.gr_image_scale_host(ctx.h, p(hin), n, pl, sh, sw, dh, dw, None if a_out is None else p(hout))
            assert rc == -1 and msg in err(), (rc, msg, err())
        dataset_cases = [  # (in, n, sh, sw, sc, dh, dw, to, normalize, out), message
            ((None, 2, 4, 4, 3, 8, 8, 0, 0, dout), "null"), ((dbytes, 2, 4, 4, 3, 8, 8, 0, 0, None), "null"),
            ((dbytes, 0, 4, 4, 3, 8, 8, 0, 0, dout), "positive"), ((dbytes, 2, 0, 4, 3, 8, 8, 0, 0, dout), "positive"),
            ((dbytes, 2, 4, 0, 3, 8, 8, 0, 0, dout), "positive"), ((dbytes, 2, 4, 4, 3, -8, 8, 0, 0, dout), "positive"),
            ((dbytes, 2, 4, 4, 3, 8, 0, 0, 0, dout), "positive"),
            ((dbytes, 2, 4, 4, 2, 8, 8, 0, 0, dout), "source channels"), ((dbytes, 2, 4, 4, 0, 8, 8, 0, 0, dout), "source channels"),
            ((dbytes, 2, 4, 4, 5, 8, 8, 0, 0, dout), "source channels"),
            ((dbytes, 2, 4, 4, 3, 8, 8, 4, 0, dout), "<to>"), ((dbytes, 2, 4, 4, 3, 8, 8, -1, 1, dout), "<to>"),
            ((dbytes, 2, 4, 4, 3, 40000, 8, 0, 0, dout), "too large"), ((dbytes, 1 << 40, 4, 4, 3, 8, 8, 0, 0, dout), "too large a batch"),
        ]
        for args, msg in dataset_cases:
            rc = ctx.lib.gr_dataset_images_dev(ctx.h, p(args[0]), *args[1:9], p(args[9]))
            assert rc == -1 and msg in err(), (rc, msg, err())
        ctx.synchronize()
        assert np.array_equal(ctx.download(dout, sentinel.shape), sentinel)
        assert np.array_equal(hout, sentinel)
        with pytest.raises(L.GanrevError, match="source channels"):
            ctx.dataset_images_dev(dbytes, 2, 4, 4, 2, 8, 8, 0, False, dout)
        with pytest.raises(L.GanrevError):
            ctx.image_scale(np.zeros((4, 4), np.float32), 8, 8)
    finally:
        ctx.free(din); ctx.free(dbytes); ctx.free(dout)


# --------------------------------------------------------------------------------------------------------------------- ganrev.dataset
def write_folder(d, n=14, sizes=((20, 24), (16, 16)), channels=(3, 1, 4)):
    """n PNG files of two source sizes and three channel counts, mixed, written by ganrev.png from synth.synthetic_images -> the decoded
    arrays in path order"""
    from ganrev import png, synth
    os.makedirs(d, exist_ok=True)
    files = {}
    for i in range(n):
        h, w = sizes[i % 3 == 1]
        c = channels[i % len(channels)]
        img = synth.synthetic_images(1, (3, h, w), 10 + i)[0] * np.linspace(0.3, 1.0, 3, dtype=np.float32)[:, None, None]
        u8 = np.ascontiguousarray((img.transpose(1, 2, 0) * 255 + 0.5).astype(np.uint8))
        u8 = u8[:, :, :1] if c == 1 else (np.concatenate([u8, np.full((h, w, 1), 99, np.uint8)], axis=2) if c == 4 else u8)
        name = "img_%02d.png" % ((11 * i) % n)                            # file order differs from creation order
        png.write_png(os.path.join(d, name), u8)
        files[os.path.join(d, name)] = u8
    return [files[k] for k in sorted(files, key=os.fsencode)]


@pytest.fixture
def DATASET():
    from ganrev import dataset
    saved = {k: getattr(dataset, k) for k in ("dirs", "fileExtension", "height", "width", "nbChannels", "colorSpace", "paths", "_seed", "_draws")}
    yield dataset
    for k, v in saved.items():
        setattr(dataset, k, v)


@pytest.mark.parametrize("space", co.SPACES)
def test_the_loader_equals_the_twin_on_a_folder_of_two_sizes(ctx, tmp_path, DATASET, space):
    from ganrev import nn_utils
    arrays = write_folder(str(tmp_path / "faces"))
    open(str(tmp_path / "faces" / "notes.txt"), "w").close()
    DATASET.setDirs([str(tmp_path / "faces")]); DATASET.setFileExtension("png"); DATASET.setColorSpace(space)
    DATASET.setHeight(12); DATASET.setWidth(12)
    res = DATASET.loadImages(1, 9999999)
    assert isinstance(res.data, nn_utils.DeviceTensor) and res.size() == len(res) == len(arrays) == 14
    assert res.indices.tolist() == list(range(14)) and res.data.shape == (14, co.PLANES[space], 12, 12)
    want = do.load_files(arrays, 12, 12, space)
    assert_bit_identical(res.data.numpy(), want, f"loadImages -> {space}")
    assert_bit_identical(res[3].numpy(), want[3], "indexing a device result")
    host = DATASET.loadImages(1, 9999999, device=False)
    assert isinstance(host.data, np.ndarray)
    assert_bit_identical(host.data, res.data.numpy(), "device=False against device=True")
    part = DATASET.loadImages(12, 50, device=False)                      # clamped to the three files from number 12 on
    assert part.indices.tolist() == [11, 12, 13]
    assert_bit_identical(part.data, want[11:], "loadImages(12, 50)")
    for seed in (1, 2):
        rnd = DATASET.loadRandomImages(9, seed=seed, normalize=True)
        assert rnd.size() == 9 and len(set(rnd.indices.tolist())) == 9
        assert_bit_identical(rnd.images.numpy(), do.load_files([arrays[i] for i in rnd.indices], 12, 12, space, True), f"loadRandomImages seed {seed}")
        assert rnd.normalize() == (0.5, 0.5)
        rh = DATASET.loadRandomImages(9, seed=seed, device=False)
        assert np.array_equal(rh.indices, rnd.indices)
        assert rh.normalize() == (0.5, 0.5)                               # host: nn_utils.normalize in place
        assert_bit_identical(rh.images, rnd.images.numpy(), "normalize() on the host against the fused step")
        rnd.free()
    res.free()


def test_the_loader_launches_once_per_group_and_honours_nbChannels(ctx, tmp_path, DATASET):
    from ganrev._lib import GanrevError
    arrays = write_folder(str(tmp_path / "one"), n=6, sizes=((16, 16), (16, 16)), channels=(3,))
    DATASET.setDirs([str(tmp_path / "one")]); DATASET.setFileExtension("png"); DATASET.setColorSpace("yuv"); DATASET.setHeight(8); DATASET.setWidth(8)
    res, kt = kernels_of(ctx, lambda: DATASET.loadImages(1, 6))
    assert [(k["kernel"], k["launches"]) for k in kt] == [("dataset_images_kernel_v4", 1)], kt
    assert_bit_identical(res.data.numpy(), do.load_files(arrays, 8, 8, "yuv"), "one size, one launch")
    res.free()
    DATASET.setNbChannels(1)
    with pytest.raises(GanrevError, match="nbChannels 1"):
        DATASET.loadImages(1, 6)
    with pytest.raises(GanrevError, match="normalize=True"):
        DATASET.setNbChannels(3)
        r = DATASET.loadImages(1, 2)
        try:
            r.normalize()
        finally:
            r.free()


def test_a_jpeg_goes_through_pillow(ctx, tmp_path, DATASET):
    Image = pytest.importorskip("PIL.Image")
    from ganrev import synth
    img = (synth.synthetic_images(1, (3, 40, 36), 3)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    Image.fromarray(img).save(str(tmp_path / "a.jpg"), quality=90)
    with Image.open(str(tmp_path / "a.jpg")) as im:
        decoded = np.asarray(im.convert("RGB"), dtype=np.uint8)
    DATASET.setDirs([str(tmp_path)]); DATASET.setFileExtension("jpg"); DATASET.setColorSpace("rgb"); DATASET.setHeight(32); DATASET.setWidth(32)
    res = DATASET.loadRandomImages(5, seed=1, device=False)
    assert res.size() == 1
    assert_bit_identical(res.images, do.dataset_images(decoded[None], 32, 32, "rgb"), "a JPEG decoded by Pillow")


# --------------------------------------------------------------------------------------------------------------------- the scripts
def test_sample_neighbours_from_a_folder_equal_those_from_the_twins_npy(ctx, tmp_path, DATASET):
    from ganrev import models, sample, synth, t7
    dims = (1, 32, 32)
    G = models.create_G(dims, 32, True, 4); synth.init_params(G, 4)
    D = models.create_D(dims, True, 5); synth.init_params(D, 5)
    t7.save_checkpoint(str(tmp_path / "adversarial.net"), G=G, D=D, opt={"width": 32, "height": 32, "colorSpace": "y"})
    arrays = write_folder(str(tmp_path / "faces"), n=40, sizes=((64, 64), (48, 40)))
    np.save(tmp_path / "twin.npy", do.load_files(arrays, 32, 32, "y"))
    argv = ["--save", str(tmp_path), "--colorSpace", "y", "--seed", "3", "--neighbours", "--runs", "1"]
    a = np.load(sample.main(argv + ["--writeTo", str(tmp_path / "a"), "--dataset", str(tmp_path / "faces"), "--fileExtension", "png", "--render"])[0])
    b = np.load(sample.main(argv + ["--writeTo", str(tmp_path / "b"), "--data", str(tmp_path / "twin.npy")])[0])
    assert a["neighbour_idx"].shape == (16,)
    for k in ("neighbour_idx", "neighbour_dist", "neighbours", "best", "best_pred"):
        assert np.array_equal(a[k], b[k]), k
    assert os.path.isfile(str(tmp_path / "a" / "trainset_s1_0001_base.png"))
    with pytest.raises(Exception, match="both"):
        sample.main(argv + ["--writeTo", str(tmp_path / "c"), "--dataset", str(tmp_path / "faces"), "--data", str(tmp_path / "twin.npy")])


def test_train_from_a_folder_writes_a_loadable_checkpoint(ctx, tmp_path, DATASET):
    from ganrev import scripts, train
    write_folder(str(tmp_path / "faces"), n=20)
    r = train.main(["--epochs", "1", "--N_epoch", "2", "--batchSize", "8", "--noiseDim", "16", "--height", "16", "--width", "16", "--colorSpace", "yuv",
                    "--dataset", str(tmp_path / "faces"), "--fileExtension", "png", "--save", str(tmp_path / "logs"), "--nopretraining", "--quiet"])
    ck = scripts.load_checkpoint(r["path"])
    assert ck["opt"]["dataset"] == str(tmp_path / "faces") and ck["opt"]["fileExtension"] == "png" and int(ck["epoch"]) == 1
    assert np.isfinite(r["last_losses"]).all()
    from ganrev._lib import GanrevError
    with pytest.raises(GanrevError, match="the loop needs"):
        train.main(["--epochs", "1", "--N_epoch", "30", "--batchSize", "8", "--noiseDim", "16", "--height", "16", "--width", "16",
                    "--dataset", str(tmp_path / "faces"), "--fileExtension", "png", "--save", str(tmp_path / "l2"), "--nopretraining", "--quiet"])
