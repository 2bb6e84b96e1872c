"""gpu: the device-resident cache of a dataset's decoded files (gr_dataset_cache_*, csrc/dataset.hip dataset_gather_kernel; ganrev.dataset.cache;
the scripts' --cacheDataset).

Every comparison is np.array_equal on the fp32 bits, against two independent sources: tests/dataset_oracle.load_files (the numpy twin of the
loader) and gr_dataset_images_dev run on each image alone.  No tolerance: the gather kernel runs the arithmetic include/ganrev.h states
operation by operation, per image, at that image's own source size.  The scripts are compared with themselves: a run with --cacheDataset
against a run without it, parameter vectors, BatchNorm running statistics and picture files byte for byte.

The error-path tests hand the library arguments its HOST-side checks refuse: nothing is launched, nothing on the device can fault."""
import ctypes as C
import os

import numpy as np
import pytest

import colorspace_oracle as co
import dataset_oracle as do
from test_gpu_colorspace import assert_bit_identical, cs, kernels_of

pytestmark = pytest.mark.gpu

# appended in this order: the unpadded sizes 3 and 105 sit in front of images that must start on a dword again
SOURCES = [(1, 1, 3),      # 3 bytes; both axes replicate
           (5, 7, 3),      # 105 bytes, no multiple of 4
           (8, 8, 1),      # a copy at an 8 x 8 target
           (20, 24, 4),    # the box average
           (3, 16, 3),     # up on one axis, down on the other
           (8, 8, 3)]
# (dh, dw, float offset of out inside its allocation) -> the store form
TARGETS = [((8, 8, 0), "dataset_gather_kernel_v4"), ((6, 5, 0), "dataset_gather_kernel"), ((8, 8, 1), "dataset_gather_kernel")]
LISTS = [list(range(6)), list(range(5, -1, -1)), [2, 2, 0, 5, 2], [3]]


def source_images():
    """uniform bytes with exact greys, 0 / 255 corners and two-way ties among the colour pixels (the hsl branches)"""
    out = []
    for k, (h, w, c) in enumerate(SOURCES):
        rng = np.random.default_rng(70 + k)
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        if c >= 3 and h * w >= 8:
            flat = a.reshape(-1, c)
            q = flat.shape[0] // 4
            flat[:q, 1] = flat[:q, 0]; flat[:q, 2] = flat[:q, 0]
            flat[q:2 * q, :3] = rng.integers(0, 2, (q, 3), dtype=np.uint8) * 255
            flat[2 * q:3 * q, 1] = flat[2 * q:3 * q, 0]
        out.append(a)
    return out


IMAGES = source_images()
_alone = {}


def alone(ctx, i, dh, dw, to, normalise):
    """gr_dataset_images_dev on image i alone (computed once per case, never changed)"""
    key = (i, dh, dw, to, normalise)
    if key not in _alone:
        a = IMAGES[i]
        din, dout = ctx.upload(a), ctx.malloc(4 * co.PLANES[to] * dh * dw)
        try:
            ctx.dataset_images_dev(din, 1, a.shape[0], a.shape[1], a.shape[2], dh, dw, cs(to), normalise, dout)
            _alone[key] = ctx.download(dout, (1, co.PLANES[to], dh, dw))
        finally:
            ctx.free(din); ctx.free(dout)
        _alone[key].setflags(write=False)
    return _alone[key]


def new_cache(ctx, chunk_bytes=0, images=IMAGES):
    import ganrev._lib as L
    cache = L.DatasetCache(ctx, chunk_bytes)
    for k, a in enumerate(images):
        assert cache.append(a) == k
    return cache


@pytest.fixture(scope="module")
def cache(ctx):
    c = new_cache(ctx)
    yield c
    c.close()


def gather(ctx, cache, idx, dh, dw, to, normalise, offset_floats=0):
    n = len(idx)
    dout = ctx.malloc(4 * (n * co.PLANES[to] * dh * dw + offset_floats))
    try:
        cache.load_dev(idx, dh, dw, cs(to), normalise, dout + 4 * offset_floats)
        return ctx.download(dout + 4 * offset_floats, (n, co.PLANES[to], dh, dw))
    finally:
        ctx.free(dout)


def test_the_cache_keeps_the_records_of_what_was_appended(ctx, cache):
    assert len(cache) == 6 and cache.size() == (6, sum(a.size for a in IMAGES))
    assert [cache.image(i) for i in range(6)] == SOURCES


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("to", co.SPACES)
def test_one_launch_writes_what_the_twin_and_the_per_image_launches_write(ctx, cache, to, normalise):
    for (dh, dw, off), label in TARGETS:
        for idx in LISTS:
            what = f"gather {idx} -> {to} {dh} x {dw} at +{4 * off} bytes, normalise {normalise}"
            got, kt = kernels_of(ctx, lambda: gather(ctx, cache, idx, dh, dw, to, normalise, off))
            assert_bit_identical(got, do.load_files([IMAGES[i] for i in idx], dh, dw, to, normalise), what + " against the twin")
            assert_bit_identical(got, np.concatenate([alone(ctx, i, dh, dw, to, normalise) for i in idx]), what + " against gr_dataset_images_dev per image")
            # ONE launch however many sizes the list mixes; its byte count: the images read plus the table written
            assert [(k["kernel"], k["launches"]) for k in kt] == [(label, 1)], (what, kt)
            assert kt[0]["bytes"] == sum(IMAGES[i].size for i in idx) + 4 * got.size, (what, kt)


def test_small_chunks_give_the_same_table(ctx, cache):
    """chunk_bytes 128: the images span several chunks, 20 x 24 x 4 (1920 bytes) gets a chunk of its own"""
    small = new_cache(ctx, 128)
    try:
        assert small.size() == cache.size()
        for to in co.SPACES:
            for (dh, dw, off), _ in TARGETS[:2]:
                for idx in (LISTS[0], LISTS[2]):
                    got = gather(ctx, small, idx, dh, dw, to, True)
                    assert_bit_identical(got, gather(ctx, cache, idx, dh, dw, to, True), f"chunk 128 against the default chunk, {idx} -> {to} {dh} x {dw}")
                    assert_bit_identical(got, do.load_files([IMAGES[i] for i in idx], dh, dw, to, True), f"chunk 128 against the twin, {idx} -> {to} {dh} x {dw}")
    finally:
        small.close()


def test_appending_after_a_load_refreshes_the_records(ctx):
    grown = new_cache(ctx, 128, IMAGES[:3])
    try:
        first = gather(ctx, grown, [2, 0, 1], 8, 8, "yuv", False)
        assert_bit_identical(first, do.load_files([IMAGES[i] for i in (2, 0, 1)], 8, 8, "yuv"), "before the append")
        for k in (3, 4, 5):
            assert grown.append(IMAGES[k]) == k
        idx = [5, 0, 3, 2, 4, 1, 3]
        for to, (dh, dw) in (("yuv", (8, 8)), ("hsl", (6, 5))):
            got, kt = kernels_of(ctx, lambda: gather(ctx, grown, idx, dh, dw, to, False))
            assert_bit_identical(got, do.load_files([IMAGES[i] for i in idx], dh, dw, to), f"old and new images together -> {to}")
            assert sum(k["launches"] for k in kt) == 1 and kt[0]["kernel"].startswith("dataset_gather_kernel"), kt
    finally:
        grown.close()


def test_bad_arguments_return_an_error_and_leave_out_untouched(ctx, cache):
    import ganrev._lib as L
    sentinel = np.full(6 * 3 * 8 * 8, 7.25, np.float32)
    dout = ctx.upload(sentinel)
    idx = np.arange(6, dtype=np.int64)
    p = lambda a: None if a is None else (C.c_void_p(a) if isinstance(a, int) else C.c_void_p(a.ctypes.data))
    err = lambda: ctx.lib.gr_last_error(ctx.h).decode()
    with_idx = lambda *v: np.array(v, dtype=np.int64)
    try:
        cases = [  # (indices, n, dh, dw, to, normalize, out), message
            ((with_idx(0, -1, 2), 3, 8, 8, 0, 0, dout), "outside"), ((with_idx(0, 6), 2, 8, 8, 0, 0, dout), "outside"),
            ((idx, 0, 8, 8, 0, 0, dout), "positive"), ((idx, -2, 8, 8, 0, 0, dout), "positive"),
            ((idx, 6, 0, 8, 0, 0, dout), "positive"), ((idx, 6, 8, -1, 0, 0, dout), "positive"),
            ((None, 6, 8, 8, 0, 0, dout), "null"), ((idx, 6, 8, 8, 0, 0, None), "null"),
            ((idx, 6, 8, 8, 4, 0, dout), "<to>"), ((idx, 6, 8, 8, -1, 1, dout), "<to>"),
            ((idx, 6, 40000, 8, 0, 0, dout), "too large"), ((idx, 1 << 40, 8, 8, 0, 0, dout), "too large a batch"),
        ]
        def refused():
            seen = []
            for a, msg in cases:
                rc = ctx.lib.gr_dataset_cache_load_dev(cache.h, p(a[0]), *a[1:6], p(a[6]))
                seen.append((rc, msg, err()))
            return seen
        seen, kt = kernels_of(ctx, refused)
        for rc, msg, text in seen:
            assert rc == -1 and msg in text, (rc, msg, text)
        assert kt == [], kt                                                   # no launch
        assert ctx.lib.gr_dataset_cache_load_dev(None, p(idx), 6, 8, 8, 0, 0, p(dout)) == -1
        ctx.synchronize()
        assert np.array_equal(ctx.download(dout, sentinel.shape), sentinel)
        # append: a channel count the loader never yields, a side of 0, a side too large, a null pointer - the cache keeps its six images
        a = np.zeros((4, 4, 2), np.uint8)
        for args, msg in (((p(a), 4, 4, 2), "source channels"), ((p(a), 0, 4, 3), "side"), ((p(a), 4, 40000, 1), "side"), ((None, 4, 4, 3), "null")):
            rc = ctx.lib.gr_dataset_cache_append(cache.h, *args)
            assert rc == -1 and msg in err(), (rc, msg, err())
        with pytest.raises(L.GanrevError, match="source channels"):
            cache.append(a)
        assert len(cache) == 6
        assert ctx.lib.gr_dataset_cache_image(cache.h, 6, None, None, None) == -1 and "outside" in err()
        assert_bit_identical(gather(ctx, cache, [1], 6, 5, "rgb", False), do.load_files([IMAGES[1]], 6, 5, "rgb"), "the cache after the refused calls")
    finally:
        ctx.free(dout)


# --------------------------------------------------------------------------------------------------------------------- ganrev.dataset
def write_faces(d, n=14, sizes=((20, 24), (16, 16)), channels=(3, 1, 4)):
    """n PNG files of two source sizes and 1 / 3 / 4 channels, mixed; the file order differs from the creation order"""
    from ganrev import png, synth
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        h, w = sizes[i % 3 == 1]
        c = channels[i % len(channels)]
        img = synth.synthetic_images(1, (3, h, w), 40 + i)[0] * np.linspace(0.4, 1.0, 3, dtype=np.float32)[:, None, None]
        u8 = np.ascontiguousarray((img.transpose(1, 2, 0) * 255 + 0.5).astype(np.uint8))
        u8 = u8[:, :, :1] if c == 1 else (np.concatenate([u8, np.full((h, w, 1), 77, np.uint8)], axis=2) if c == 4 else u8)
        png.write_png(os.path.join(d, "face_%02d.png" % ((5 * i) % n)), u8)
    return d


@pytest.fixture
def DATASET():
    from ganrev import dataset
    keys = ("dirs", "fileExtension", "height", "width", "nbChannels", "colorSpace", "paths", "_seed", "_draws")
    dataset.uncache()
    saved = {k: getattr(dataset, k) for k in keys}
    yield dataset
    dataset.uncache()
    for k, v in saved.items():
        setattr(dataset, k, v)


def host(images):
    from ganrev import nn_utils
    return images.numpy() if isinstance(images, nn_utils.DeviceTensor) else images


def open_faces(DATASET, d, space="yuv", size=(12, 12)):
    DATASET.setDirs([d]); DATASET.setFileExtension("png"); DATASET.setColorSpace(space); DATASET.setNbChannels(None)
    DATASET.setHeight(size[0]); DATASET.setWidth(size[1])


LOADS = [lambda D, **k: D.loadImages(1, 14, **k), lambda D, **k: D.loadImages(5, 4, **k), lambda D, **k: D.loadRandomImages(9, seed=3, **k)]


def test_cached_loads_equal_the_uncached_loads(ctx, tmp_path, DATASET):
    from ganrev import nn_utils
    open_faces(DATASET, write_faces(str(tmp_path / "faces")))
    kwargs = [dict(device=True), dict(device=False), dict(device=True, normalize=True), dict(device=False, normalize=True)]
    plain = [[load(DATASET, **k) for k in kwargs] for load in LOADS]
    assert DATASET.cache() == 14 and DATASET.cached()
    for load, wants in zip(LOADS, plain):
        for k, want in zip(kwargs, wants):
            got, kt = kernels_of(ctx, lambda: load(DATASET, **k))
            assert isinstance(got.data, nn_utils.DeviceTensor) == k["device"] and got.size() == want.size()
            assert np.array_equal(got.indices, want.indices) and got.paths == want.paths
            assert_bit_identical(host(got.images), host(want.images), f"cached against uncached, {k}")
            # two sizes and three channel counts in the folder: still one launch, and no grouped launch of the uncached path
            assert [(t["kernel"], t["launches"]) for t in kt] == [("dataset_gather_kernel_v4", 1)], kt
            if not k["device"]:
                assert got.normalize() == want.normalize() == (0.5, 0.5)
                assert_bit_identical(got.images, want.images, "normalize() on host results")
            got.free(); want.free()


def test_unseeded_draws_follow_the_same_stream(ctx, tmp_path, DATASET):
    open_faces(DATASET, write_faces(str(tmp_path / "faces")))
    DATASET.setSeed(11)
    plain = [DATASET.loadRandomImages(6, device=False) for _ in range(2)]
    DATASET.cache()
    DATASET.setSeed(11)
    again = [DATASET.loadRandomImages(6, device=False) for _ in range(2)]
    assert not np.array_equal(plain[0].indices, plain[1].indices)
    for a, b in zip(plain, again):
        assert np.array_equal(a.indices, b.indices) and a.paths == b.paths
        assert_bit_identical(b.images, a.images, "an unseeded draw")


def test_a_colour_file_under_nbChannels_1_is_refused_the_same_way(ctx, tmp_path, DATASET):
    from ganrev._lib import GanrevError
    open_faces(DATASET, write_faces(str(tmp_path / "faces")))
    DATASET.setNbChannels(1)
    with pytest.raises(GanrevError, match="nbChannels 1") as plain:
        DATASET.loadImages(1, 14)
    DATASET.cache()

    def refused():
        with pytest.raises(GanrevError, match="nbChannels 1") as cached:
            DATASET.loadImages(1, 14)
        return str(cached.value)
    text, kt = kernels_of(ctx, refused)
    assert text == str(plain.value)
    assert kt == [], kt                                                       # refused from the host records, before any launch


def test_the_cache_outlives_the_target_settings_and_goes_with_the_files(ctx, tmp_path, DATASET):
    d = write_faces(str(tmp_path / "faces"))
    open_faces(DATASET, d)
    plain = {}
    for space, size in (("hsl", (9, 10)), ("y", (16, 8)), ("rgb", (12, 12))):
        DATASET.setColorSpace(space); DATASET.setHeight(size[0]); DATASET.setWidth(size[1])
        plain[space] = DATASET.loadImages(1, 14, device=False).images
    DATASET.cache()
    for space, size in (("hsl", (9, 10)), ("y", (16, 8)), ("rgb", (12, 12))):
        DATASET.setColorSpace(space); DATASET.setHeight(size[0]); DATASET.setWidth(size[1]); DATASET.setNbChannels(3)
        assert DATASET.cached()
        got = DATASET.loadImages(1, 14, device=False).images
        assert got.shape == (14, co.PLANES[space]) + size
        assert_bit_identical(got, plain[space], f"after the setters -> {space} {size}")
    DATASET.setFileExtension("png")
    assert not DATASET.cached()
    DATASET.cache()
    DATASET.setDirs([d])
    assert not DATASET.cached()
    res, kt = kernels_of(ctx, lambda: DATASET.loadImages(1, 14, device=False))
    assert_bit_identical(res.images, plain["rgb"], "uncached again")
    assert all(t["kernel"].startswith("dataset_images_kernel") for t in kt) and kt, kt
    DATASET.cache(); DATASET.uncache()
    assert not DATASET.cached()


# --------------------------------------------------------------------------------------------------------------------- the scripts
SMALL = ["--batchSize", "4", "--noiseDim", "8", "--height", "16", "--width", "16", "--quiet"]      # the smallest geometry the models accept


def _flat(model):
    return model._flat_host() if model._flat is None else model._flat[0].copy()


def _bn(model):
    return [a for m in model.leaves() if hasattr(m, "running_mean") for a in (m.running_mean, m.running_var)]


def same_checkpoints(path_a, path_b, keys):
    """parameter vectors and BatchNorm running statistics bit for bit; the opt tables differ in cacheDataset and the save directory alone"""
    from ganrev import t7
    a, b = t7.load_checkpoint(path_a), t7.load_checkpoint(path_b)
    for k in keys:
        assert _flat(a[k]).size > 0 and np.array_equal(_flat(a[k]), _flat(b[k])), f"{k}: parameters"
        assert len(_bn(a[k])) == len(_bn(b[k])) and all(np.array_equal(p, q) for p, q in zip(_bn(a[k]), _bn(b[k]))), f"{k}: BatchNorm running statistics"
    assert "cacheDataset" not in a["opt"] and b["opt"]["cacheDataset"] == True  # noqa: E712  (the saved scalar)
    strip = lambda o: {k: v for k, v in o.items() if k not in ("cacheDataset", "save")}
    assert strip(a["opt"]) == strip(b["opt"])


def test_train_draws_the_same_images_from_the_cache(ctx, tmp_path, DATASET, capsys):
    from ganrev import train
    d = write_faces(str(tmp_path / "faces"))
    args = SMALL + ["--epochs", "2", "--N_epoch", "2", "--colorSpace", "yuv", "--saveFreq", "100", "--nopretraining", "--dataset", d, "--fileExtension", "png"]
    plain = train.main(args + ["--save", str(tmp_path / "plain")])
    assert not DATASET.cached()
    cached = train.main(args + ["--save", str(tmp_path / "cached"), "--cacheDataset"])
    assert DATASET.cached() and plain["last_losses"] == cached["last_losses"]
    same_checkpoints(plain["path"], cached["path"], ("G", "D"))
    capsys.readouterr()
    train.main([a for a in args if a != "--quiet"] + ["--save", str(tmp_path / "loud"), "--cacheDataset"])
    assert capsys.readouterr().out.count("caching 14 files") == 1             # once, not per epoch


def test_train_progress_pictures_are_the_same_files(ctx, tmp_path, DATASET):
    from ganrev import train
    d = write_faces(str(tmp_path / "faces"))
    args = SMALL + ["--epochs", "2", "--N_epoch", "2", "--colorSpace", "rgb", "--saveFreq", "100", "--nopretraining", "--dataset", d, "--fileExtension", "png",
                    "--progress"]
    plain = train.main(args + ["--save", str(tmp_path / "plain")])
    cached = train.main(args + ["--save", str(tmp_path / "cached"), "--cacheDataset"])
    same_checkpoints(plain["path"], cached["path"], ("G", "D"))
    for kind in ("images", "images_good", "images_bad", "images_train"):
        for epoch in (1, 2):
            a, b = (open(str(tmp_path / run / kind / ("%d_%05d.png" % (r["pictures"].start, epoch))), "rb").read()
                    for run, r in (("plain", plain), ("cached", cached)))
            assert len(a) > 100 and a == b, (kind, epoch)


def test_pretrain_g_draws_the_same_images_from_the_cache(ctx, tmp_path, DATASET):
    from ganrev import pretrain_g
    d = write_faces(str(tmp_path / "faces"))
    for space in ("y", "yuv"):                                                # y: a table of its own after the conversion; yuv: converted in place
        args = SMALL + ["--epochs", "2", "--N_epoch", "2", "--colorSpace", space, "--saveFreq", "100", "--dataset", d, "--fileExtension", "png"]
        plain = pretrain_g.main(args + ["--save", str(tmp_path / (space + "_plain"))])
        cached = pretrain_g.main(args + ["--save", str(tmp_path / (space + "_cached")), "--cacheDataset"])
        assert plain["last_loss"] == cached["last_loss"]
        same_checkpoints(plain["path"], cached["path"], ("G",))
        assert np.array_equal(_flat(plain["model"]), _flat(cached["model"]))  # the encoder too


def test_pretrain_with_previous_net_draws_the_same_images_from_the_cache(ctx, tmp_path, DATASET):
    from ganrev import pretrain_with_previous_net as P
    from ganrev import train
    d = write_faces(str(tmp_path / "faces"))
    prev = train.main(SMALL + ["--epochs", "1", "--N_epoch", "1", "--colorSpace", "gray", "--save", str(tmp_path / "prev")])["path"]
    args = SMALL + ["--network", prev, "--N_batches", "3", "--colorSpace", "y", "--saveFreq", "100", "--dataset", d, "--fileExtension", "png"]
    plain = P.main(args + ["--save", str(tmp_path / "plain")])
    cached = P.main(args + ["--save", str(tmp_path / "cached"), "--cacheDataset"])
    assert plain["last_losses"] == cached["last_losses"]
    same_checkpoints(plain["path"], cached["path"], ("G", "D"))


def test_sample_finds_the_same_neighbours_in_the_cache(ctx, tmp_path, DATASET):
    from ganrev import models, sample, synth, t7
    dims = (1, 32, 32)
    G = models.create_G(dims, 32, True, 4); synth.init_params(G, 4)
    D = models.create_D(dims, True, 5); synth.init_params(D, 5)
    t7.save_checkpoint(str(tmp_path / "adversarial.net"), G=G, D=D, opt={"width": 32, "height": 32, "colorSpace": "y"})
    d = write_faces(str(tmp_path / "faces"), n=20)
    argv = ["--save", str(tmp_path), "--colorSpace", "y", "--seed", "3", "--neighbours", "--runs", "1", "--dataset", d, "--fileExtension", "png", "--render"]
    a = np.load(sample.main(argv + ["--writeTo", str(tmp_path / "a")])[0])
    b = np.load(sample.main(argv + ["--writeTo", str(tmp_path / "b"), "--cacheDataset"])[0])
    assert DATASET.cached() and a["neighbour_idx"].shape == (16,)
    for k in ("neighbour_idx", "neighbour_dist", "neighbours", "best", "best_pred"):
        assert np.array_equal(a[k], b[k]), k
    name = "trainset_s1_0001_base.png"                                        # the 64 random training images, drawn from the cache
    assert open(str(tmp_path / "a" / name), "rb").read() == open(str(tmp_path / "b" / name), "rb").read()
