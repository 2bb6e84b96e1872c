"""gpu: python -m ganrev.apply_r reads --dataset - search by example with the dataset's first files as needles (--needles) and the dataset's
images as the corpus (--real).  The folder is 520 tiny uint8 .npy images (no Pillow needed) of two source sizes; the nets are --synthetic."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SYN, BATCH, SEED = "1x32x32x32", 64, 1
DIMS, ND = (1, 32, 32), 32


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("faces")
    rng = np.random.default_rng(11)
    for i in range(520):
        h, w = (32, 32) if i % 3 else (24, 28)
        base = rng.integers(0, 256, size=(h // 4, w // 4), dtype=np.uint8)
        img = np.kron(base, np.ones((4, 4), np.uint8)) // 2 + rng.integers(0, 128, size=(h, w), dtype=np.uint8)
        np.save(d / ("face_%03d.npy" % ((7 * i) % 520)), img.astype(np.uint8)[:, :, None])
    return str(d)


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


def run(tmp_path, name, extra):
    from ganrev import apply_r
    out = tmp_path / name
    apply_r.main(["--synthetic", SYN, "--batchSize", str(BATCH), "--seed", str(SEED), "--quiet", "--writeTo", str(out)] + extra)
    arrays = {f: np.load(out / f) for f in sorted(os.listdir(out)) if f.endswith(".npy")}
    return arrays, json.load(open(out / "summary.json")), out


def reverser(ctx):
    """MODEL_R as apply_r.main builds it for --synthetic"""
    from ganrev import models, synth
    R = models.create_R(DIMS, ND, "normal", False, seed=SEED + 1); synth.init_params(R, SEED + 1)
    R._ctx = ctx
    R.evaluate()
    return R


def first_images(DATASET, ctx, folder, n):
    DATASET.setColorSpace("y"); DATASET.setFileExtension("npy"); DATASET.setHeight(32); DATASET.setWidth(32); DATASET.setDirs([folder])
    return DATASET.loadImages(1, n, ctx=ctx)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_needles_from_the_dataset(ctx, tmp_path, folder, DATASET):
    from ganrev import nn_utils
    ds = ["--dataset", folder, "--fileExtension", "npy"]
    plain, s_plain, _ = run(tmp_path, "plain", ["--nbImages", "600"] + ds)
    got, s_got, out = run(tmp_path, "needles", ["--nbImages", "600", "--needles", "3", "--render"] + ds)
    cached, s_cached, _ = run(tmp_path, "cached", ["--nbImages", "600", "--needles", "3", "--cacheDataset"] + ds)
    # a run without the option is what it was: no new file, no new key; and the option changes nothing the run wrote before
    assert "needles" not in s_plain and not [f for f in plain if f.startswith("needle")]
    assert set(got) - set(plain) == {"needle_by_attributes.npy", "needle_by_pixels.npy", "needle_attributes.npy"}
    for f in ("attributes.npy", "similar_by_attributes.npy", "attributes_fixer.npy", "similar_by_pixels.npy"):
        assert same(plain[f], got[f]) and same(plain[f], cached[f]), f
    assert set(s_got) - set(s_plain) == {"needles"} and s_got["needles"]["count"] == 3
    assert s_got["needles"]["files"] == ["face_000.npy", "face_001.npy", "face_002.npy"]
    # the needle attributes are R over DATASET.loadImages(1, 3), bit for bit
    res = first_images(DATASET, ctx, folder, 3)
    want = nn_utils.forwardBatchedDev(reverser(ctx), res.images, BATCH)
    assert same(got["needle_attributes.npy"], want.numpy())
    # the lists are the search by example over the saved tables
    idx, _ = ctx.cosine_topk_queries(got["attributes.npy"], got["needle_attributes.npy"], 100)
    assert got["needle_by_attributes.npy"].shape == (3, 100) and np.array_equal(got["needle_by_attributes.npy"], idx)
    # (the corpus images are not saved: the pixel lists are checked for shape and range here, against the row-index search in the --real test)
    assert got["needle_by_pixels.npy"].shape == (3, 100) and got["needle_by_pixels.npy"].min() >= 0 and got["needle_by_pixels.npy"].max() < 600
    want.free(); res.free()
    # with and without --cacheDataset: the same bits
    for f in ("needle_by_attributes.npy", "needle_by_pixels.npy", "needle_attributes.npy"):
        assert same(got[f], cached[f]), f
    assert not DATASET.cached(), "the run gives the cache back"
    for i in (1, 2, 3):
        assert os.path.getsize(out / ("needle_attributes_%02d.png" % i)) > 0 and os.path.getsize(out / ("needle_pixelwise_%02d.png" % i)) > 0
    # --refine refines the needles against themselves, like the corpus
    ref, s_ref, _ = run(tmp_path, "refined", ["--nbImages", "520", "--needles", "3", "--refine", "2"] + ds)
    r = s_ref["needles"]["refine"]
    assert r["steps"] == 2 and r["loss_after_mean"] <= r["loss_before_mean"] and 0 <= r["rows_improved"] <= 3
    assert ref["needle_attributes.npy"].shape == (3, ND) and (r["rows_improved"] == 0 or not same(ref["needle_attributes.npy"], got["needle_attributes.npy"]))


def test_real_images_as_the_corpus(ctx, tmp_path, folder, DATASET):
    from ganrev import apply_r, nn_utils
    from ganrev._lib import GanrevError
    ds = ["--dataset", folder, "--fileExtension", "npy"]
    got, s, _ = run(tmp_path, "real", ["--nbImages", "520", "--real", "--resident"] + ds)
    res = first_images(DATASET, ctx, folder, 520)
    want = nn_utils.forwardBatchedDev(reverser(ctx), res.images, BATCH)
    assert same(got["attributes.npy"], want.numpy()), "attributes = R over the dataset's first 520 images"
    rows = np.array([99, 199, 299, 399, 499], dtype=np.int64)
    idx, _ = ctx.cosine_topk(got["attributes.npy"], rows, 100)
    assert np.array_equal(got["similar_by_attributes.npy"], idx)
    pidx, _ = ctx.cosine_topk(res.images.numpy().reshape(520, -1), rows, 100)
    assert np.array_equal(got["similar_by_pixels.npy"], pidx)
    want.free(); res.free()
    assert s["corpus"] == "dataset" and s["path"] == "device-resident" and got["variations.npy"].shape[0] == ND
    # --refine: the refinement of real images through G
    ref, s_ref, _ = run(tmp_path, "refined", ["--nbImages", "520", "--real", "--resident", "--refine", "3"] + ds)
    r = s_ref["refine"]
    assert r["steps"] == 3 and r["loss_after_mean"] <= r["loss_before_mean"] and 0 <= r["rows_improved"] <= 520
    assert same(ref["attributes_fixer.npy"], got["attributes_fixer.npy"])
    # fewer files than --nbImages
    with pytest.raises(GanrevError, match="520.*521"):
        apply_r.main(["--synthetic", SYN, "--batchSize", str(BATCH), "--quiet", "--writeTo", str(tmp_path / "short"), "--nbImages", "521", "--real"] + ds)
