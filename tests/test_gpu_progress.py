"""gpu: the trainers' progress pictures.  gr_progress_grid_dev against its numpy restatement (tests/progress_oracle.py; the colour step
through gr_colorspace_host), np.array_equal on both outputs; every argument the call refuses; the forward-counter round trip that
ganrev.progress.observing rests on; and the claim the feature stands on - a run with --progress saves, bit for bit, the checkpoint of a
run without it - for the four trainers, with the content of train's pictures rebuilt by the host route.

The error-path tests hand the library arguments its HOST-side checks refuse: nothing is launched, nothing on the device can fault."""
import json
import os

import numpy as np
import pytest

import progress_oracle as po

pytestmark = pytest.mark.gpu
F = np.float32
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
SMALL = ["--batchSize", "4", "--noiseDim", "8", "--height", "16", "--width", "16", "--quiet"]      # the smallest geometry the models accept


# ---------------------------------------------------------------------------------------------------------------- the grid kernel
def table_of(n, c, h, w, seed):
    """values from -0.25 to 1.25: below 0 and above 1, for the u8 clamp"""
    return np.random.default_rng(seed).uniform(-0.25, 1.25, (n, c, h, w)).astype(F)


def run_grid(ctx, table, rows, grid_h, grid_w, epoch, from_space, n_show=None, offset=0, want=("grid", "u8")):
    n, c, h, w = table.shape
    cout, gh, gw = po.shape(c, h, w, from_space, grid_h, grid_w)
    base = ctx.malloc(table.nbytes + offset)
    gd = ctx.malloc(4 * cout * gh * gw) if "grid" in want else None
    ud = ctx.malloc(cout * gh * gw) if "u8" in want else None
    try:
        ctx.upload(table, base + offset)
        assert ctx.progress_grid_dev(base + offset, n, c, h, w, from_space, rows, grid_h, grid_w, epoch, gd, ud, n_show=n_show) == (cout, gh, gw)
        return (ctx.download(gd, (cout, gh, gw), F) if gd else None), (ctx.download(ud, (gh, gw, cout), np.uint8) if ud else None)
    finally:
        for p in (base, gd, ud):
            if p:
                ctx.free(p)


def check_grid(ctx, table, rows, grid_h, grid_w, epoch, from_space, n_show=None, **kw):
    import ganrev._lib as L
    g, u = run_grid(ctx, table, rows, grid_h, grid_w, epoch, from_space, n_show, **kw)
    want = po.progress_grid(table, rows, len(rows) if n_show is None else n_show, grid_h, grid_w, epoch, from_space,
                            to_rgb=lambda t: t if from_space == L.GR_CS_RGB else ctx.colorspace(t, from_space, L.GR_CS_RGB))
    if g is not None:
        assert g.dtype == want.dtype and np.array_equal(g.view(np.uint32), want.view(np.uint32))
    if u is not None:
        assert np.array_equal(u, po.quantise(want))
    return want


ROWS = [5, 2, 2, 6, 0, 5, 3, 1, 4]            # repeated and out of order


@pytest.mark.parametrize("from_space", [0, 1, 2, 3, -1])
def test_grid_scalar_path_every_colour_space(ctx, from_space):
    """w = 5: no four pixels of a row share alignment, one pixel per thread.  2 x 3 grids; n_show 0, 4, 6 and 9: an empty grid, empty
    cells, a full grid, extras that are ignored; epochs of one and two digits"""
    table = table_of(7, 1 if from_space == 1 else 3, 4, 5, 20 + from_space)
    for n_show, epoch in ((0, 0), (4, 7), (6, 10), (9, 7)):
        want = check_grid(ctx, table, ROWS, 2, 3, epoch, from_space, n_show)
        assert want.shape == (3 if from_space >= 0 else table.shape[1], 15, 15)
        assert not want[:, 13:].any() and want[:, 8:13, 7:10].any() and not want[:, 8:13, 10:].any()   # below the cells: the digits, rows 8 .. 12


def test_grid_one_channel_copied_as_it_is(ctx):
    table = table_of(7, 1, 4, 5, 3)
    table[2, 0, 1, 3] = np.nan                                   # a NaN travels as it is into the float grid and gives byte 0
    want = check_grid(ctx, table, ROWS, 2, 3, 10, -1, 6)
    assert want.shape == (1, 15, 15) and np.isnan(want[0, 1, 8])


@pytest.mark.parametrize("from_space", [0, 1, 2, 3, -1])
def test_grid_vector_path(ctx, from_space):
    """w = 8, grid_w = 4: GW = 32, four pixels per thread - and the smallest width that takes the five digits of epoch 12345.  The same
    call on a table 4 bytes off its allocation takes the scalar path and must give the same picture."""
    table = table_of(7, 1 if from_space == 1 else 3, 4, 8, 40 + from_space)
    for offset in (0, 4):
        check_grid(ctx, table, ROWS, 2, 4, 12345, from_space, 6, offset=offset)
    check_grid(ctx, table, ROWS, 2, 4, 0, from_space, 9, want=("u8",))
    check_grid(ctx, table, ROWS, 2, 4, 7, from_space, 4, want=("grid",))
    if from_space == -1:
        check_grid(ctx, table_of(7, 1, 4, 8, 9), ROWS, 2, 4, 12345, -1, 9)       # one channel: the u8 word holds four pixels


def test_grid_more_than_one_block(ctx):
    """10 x 10 cells of 3 x 16 x 16: 167 x 160 pixels, 27 workgroups of the vector kernel"""
    check_grid(ctx, table_of(100, 3, 16, 16, 5), np.random.default_rng(1).permutation(100), 10, 10, 31, 2)


def test_grid_refuses_bad_arguments_and_writes_nothing(ctx):
    import ganrev._lib as L
    table = table_of(4, 3, 4, 5, 1)
    td, gd, ud = ctx.upload(table), ctx.malloc(4 * 3 * 15 * 40), ctx.malloc(3 * 15 * 40)
    sentinel_g, sentinel_u = np.full(3 * 15 * 40, 7.0, F), np.full(3 * 15 * 40, 0xAB, np.uint8)
    ctx.upload(sentinel_g, gd); ctx.upload(sentinel_u, ud)
    ok = dict(table_dev=td, n_rows=4, channels=3, h=4, w=5, from_space=0, rows=[0, 1, 2, 3], grid_h=2, grid_w=3, epoch=1, grid_dev=gd, u8_dev=ud)
    bad = [dict(table_dev=None), dict(grid_dev=None, u8_dev=None),
           dict(channels=2), dict(channels=3, from_space=1), dict(channels=1, from_space=2), dict(from_space=4), dict(from_space=-2),
           dict(h=0), dict(w=0), dict(grid_h=0), dict(grid_w=0), dict(n_show=-1), dict(n_rows=0),
           dict(rows=[0, 4, 1]), dict(rows=[0, -1]), dict(epoch=-1),
           dict(w=19, grid_w=1, epoch=100),                      # GW = 19: 19 - 2 - 18 < 0
           dict(h=16384, w=16384, grid_h=1, grid_w=2, rows=[], epoch=1)]      # 16391 x 32768 pixels > 2^28
    try:
        for change in bad:
            with pytest.raises(L.GanrevError, match="GR_ERR_INVALID|INVALID") as e:
                ctx.progress_grid_dev(**dict(ok, **change))
            assert "gr_progress_grid_dev" in str(e.value), change
        assert np.array_equal(ctx.download(gd, sentinel_g.shape, F), sentinel_g) and np.array_equal(ctx.download(ud, sentinel_u.shape, np.uint8), sentinel_u)
        # the accepted neighbours: epoch 100 at GW = 20, and a bad row beyond the grid, which is ignored
        ctx.progress_grid_dev(**dict(ok, w=20, grid_w=1, grid_h=1, rows=[0], epoch=100, table_dev=td, h=1))
        ctx.progress_grid_dev(**dict(ok, grid_h=1, grid_w=2, rows=[0, 1, 999]))
        ctx.synchronize()
    finally:
        for p in (td, gd, ud):
            ctx.free(p)


# ---------------------------------------------------------------------------------------------------------------- the forward counter
def test_forward_counter_round_trip_keeps_the_dropout_masks(ctx):
    """forward A; counter read; an evaluate forward; counter set back: the next training forward draws the masks of a twin net that never
    ran the evaluate forward.  Without the set-back they differ (so the first half cannot pass vacuously)."""
    import ganrev._lib as L
    from ganrev import models, synth
    x = synth.uniform((4, 1, 16, 16), 1, 0, 1)

    def make():
        R = models.create_R((1, 16, 16), 8, seed=3)
        synth.init_params(R, 2)
        R.training(); R.manualSeed(5)
        R.forward(x)                                             # forward A
        return R

    def masks(R):
        R.training(); R.forward(x)
        return [R.getNoise(m, 4) for m in R.leaves() if m.typename in ("nn.Dropout", "nn.SpatialDropout")]

    def look(R):
        R._net.set_training(False)
        R._net.forward(x)
        R._net.set_training(True)

    observed, twin, disturbed = make(), make(), make()
    assert observed._net.forward_counter() == twin._net.forward_counter() == 1
    counter = observed._net.forward_counter()
    look(observed)
    assert observed._net.forward_counter() == counter + 1
    observed._net.set_forward_counter(counter)
    assert observed._net.forward_counter() == counter
    look(disturbed)
    want, got, other = masks(twin), masks(observed), masks(disturbed)
    assert len(want) >= 2 and all(0 < m.mean() < 1 for m in want)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert any(not np.array_equal(a, b) for a, b in zip(other, want))
    assert observed._net.forward_counter() == twin._net.forward_counter() == 2 and disturbed._net.forward_counter() == 3
    with pytest.raises(L.GanrevError):
        observed._net.set_forward_counter(-1)
    assert observed._net.forward_counter() == 2


def test_observing_restores_mode_and_counters_of_models_and_plain_nets(ctx):
    from ganrev import device, models, progress, synth
    R = models.create_R((1, 16, 16), 8, seed=3)
    R.training(); R.forward(synth.uniform((2, 1, 16, 16), 1, 0, 1))
    D = models.create_D((1, 16, 16), True, 1)
    D.training(); D.forward(synth.uniform((2, 1, 16, 16), 1, 0, 1))
    dm = device.DeviceModel(ctx, D)
    x = ctx.upload(synth.uniform((2, 1, 16, 16), 2, 0, 1))
    try:
        before = [n.forward_counter() for n in dm.nets + [R._net]]
        with progress.observing(dm, R._net):
            assert not any(n.training for n in dm.nets + [R._net])
            dm.forward(x, 2); R._net.forward_dev(x, 2)
            assert [n.forward_counter() for n in dm.nets + [R._net]] == [c + 1 for c in before]
        assert all(n.training for n in dm.nets + [R._net]) and [n.forward_counter() for n in dm.nets + [R._net]] == before
    finally:
        ctx.free(x); dm.close()


# ---------------------------------------------------------------------------------------------------------------- the four trainers
def _flat(model):
    return model._flat_host() if model._flat is None else model._flat[0].copy()


def _bn(model):
    return [a for m in model.leaves() if hasattr(m, "running_mean") for a in (m.running_mean, m.running_var)]


def same_models(path_a, path_b, keys):
    from ganrev import t7
    a, b = t7.load_checkpoint(path_a), t7.load_checkpoint(path_b)
    for k in keys:
        assert _flat(a[k]).size > 0 and np.array_equal(_flat(a[k]), _flat(b[k])), f"{k}: parameters"
        assert len(_bn(a[k])) == len(_bn(b[k])) and all(np.array_equal(p, q) for p, q in zip(_bn(a[k]), _bn(b[k]))), f"{k}: BatchNorm running statistics"
    return a, b


def png_size(path):
    data = open(path, "rb").read()
    assert data[:8] == PNG_SIGNATURE, path
    return int.from_bytes(data[20:24], "big"), int.from_bytes(data[16:20], "big")       # (height, width)


def plot_rows(save, script, n_values):
    doc = json.load(open(os.path.join(save, "plot_data.json")))
    assert doc["script"] == script and all(len(r) == n_values == len(doc["labels"]) for r in doc["data"])
    return doc["data"]


def test_train_with_pictures_saves_the_same_checkpoint(ctx, tmp_path):
    from ganrev import train
    args = SMALL + ["--epochs", "2", "--N_epoch", "2", "--colorSpace", "gray", "--saveFreq", "100"]
    plain = train.main(args + ["--save", str(tmp_path / "plain")])
    seen = train.main(args + ["--save", str(tmp_path / "seen"), "--progress"])
    assert plain["pictures"] is None and plain["last_losses"] == seen["last_losses"]
    a, b = same_models(plain["path"], seen["path"], ("G", "D"))
    assert "vis_noise_inputs" not in a and "progress" not in a["opt"] and sorted(os.listdir(tmp_path / "plain")) == ["adversarial.net"]
    assert np.array_equal(b["vis_noise_inputs"], seen["pictures"].vis_noise_inputs) and b["vis_noise_inputs"].shape == (100, 8)
    assert [list(map(float, r)) for r in b["plot_data"]] == [list(map(float, r)) for r in seen["pictures"].plot_data] and len(b["plot_data"]) == 2
    start = seen["pictures"].start
    for kind, size in (("images", (167, 160)), ("images_good", (119, 112)), ("images_bad", (119, 112)), ("images_train", (135, 112))):
        for epoch in (1, 2):
            assert png_size(str(tmp_path / "seen" / kind / ("%d_%05d.png" % (start, epoch)))) == size
    rows = plot_rows(str(tmp_path / "seen"), "train", 3)
    assert [r[0] for r in rows] == [1.0, 2.0] and rows[1][1:] == [float(v) for v in seen["last_losses"]]


def test_pretrain_g_with_pictures_saves_the_same_checkpoint(ctx, tmp_path):
    from ganrev import pretrain_g
    args = SMALL + ["--epochs", "2", "--N_epoch", "2", "--colorSpace", "y", "--saveFreq", "100"]
    plain = pretrain_g.main(args + ["--save", str(tmp_path / "plain")])
    seen = pretrain_g.main(args + ["--save", str(tmp_path / "seen"), "--progress"])
    assert plain["last_loss"] == seen["last_loss"]
    same_models(plain["path"], seen["path"], ("G",))
    assert np.array_equal(_flat(plain["model"]), _flat(seen["model"]))                  # the encoder too
    for kind in ("real", "decoded"):
        for epoch in (1, 2):
            assert png_size(str(tmp_path / "seen" / "progress" / ("%s_%05d.png" % (kind, epoch)))) == (23, 160)
    assert [r[0] for r in plot_rows(str(tmp_path / "seen"), "pretrain_g", 2)] == [1.0, 2.0]
    assert sorted(os.listdir(tmp_path / "plain")) == [os.path.basename(plain["path"])]


def test_pretrain_with_previous_net_with_pictures_saves_the_same_checkpoint(ctx, tmp_path):
    """10 batches: visualizeProgress is due once, at batch 10"""
    from ganrev import pretrain_with_previous_net as P
    from ganrev import train
    prev = train.main(SMALL + ["--epochs", "1", "--N_epoch", "1", "--colorSpace", "gray", "--save", str(tmp_path / "prev")])["path"]
    args = SMALL + ["--network", prev, "--N_batches", "10", "--colorSpace", "y", "--saveFreq", "100"]
    plain = P.main(args + ["--save", str(tmp_path / "plain")])
    seen = P.main(args + ["--save", str(tmp_path / "seen"), "--progress"])
    assert plain["last_losses"] == seen["last_losses"]
    same_models(plain["path"], seen["path"], ("G", "D"))
    for kind, size in (("images", (167, 160)), ("good", (87, 160)), ("bad", (87, 160))):
        assert png_size(str(tmp_path / "seen" / "progress" / ("%s_00010.png" % kind))) == size
    assert sorted(os.listdir(tmp_path / "seen")) == sorted(os.listdir(tmp_path / "plain") + ["progress"])


def test_train_r_with_pictures_saves_the_same_checkpoint(ctx, tmp_path):
    """26 batches: the pairs picture is due once, at batch 25"""
    from ganrev import train_r
    args = ["--batchSize", "4", "--noiseDim", "8", "--height", "16", "--width", "16", "--channels", "1", "--nbBatches", "26", "--quiet"]
    _, _, plain = train_r.main(args + ["--save", str(tmp_path / "plain")])
    _, _, seen = train_r.main(args + ["--save", str(tmp_path / "seen"), "--progress"])
    assert len(plain) == 26 and plain == seen
    name = "r_1x16x16_nd8_normal.net"
    same_models(str(tmp_path / "plain" / name), str(tmp_path / "seen" / name), ("R",))
    assert png_size(str(tmp_path / "seen" / "progress" / "pairs_00025.png")) == (23, 160)           # 8 cells in a row of 10
    assert plot_rows(str(tmp_path / "seen"), "train_r", 4) == []                                     # the first row comes at batch 100
    assert sorted(os.listdir(tmp_path / "seen")) == sorted([name, "progress", "plot_data.json"])


# ---------------------------------------------------------------------------------------------------------------- what train's pictures show
@pytest.mark.parametrize("colorSpace", ["gray", "yuv"])
def test_train_pictures_equal_the_host_route(ctx, tmp_path, colorSpace):
    """The same pictures by the host route: the parameters pulled, host mirrors of G and D in evaluate(), forwardBatched with the same
    --batchSize, predictionOrder, the numpy grid.  Bit for bit: the evaluate()-mode device forward and the host-tensor forward run the same
    kernels on the same batches."""
    import ganrev._lib as L
    from ganrev import adversarial, models, nn_utils, progress, scripts, synth, t7
    dims = scripts.image_dims(colorSpace, 16, 16)
    B, nd, seed, epoch = 4, 8, 1, 3
    D, G = models.create_D(dims, True, seed), models.create_G(dims, nd, True, seed + 1)
    env = adversarial.make_env(G, D, dims, batchSize=B, N_epoch=2, noiseDim=nd, seed=seed)
    game = adversarial.DeviceGame(env)
    TRAIN_DATA = synth.uniform((60,) + dims, 5, 0, 1)
    for b in range(2):                                           # a model that has moved, Dropout counters that have ticked
        game.batch(TRAIN_DATA[2 * b:2 * b + 2])
    pictures = progress.TrainPictures(game, dims, colorSpace, str(tmp_path), start=7)
    try:
        out = pictures.visualize(TRAIN_DATA, epoch)
        ranked = ctx.download(pictures.ranked, (100,) + dims)
        vis = pictures.vis_noise_inputs.copy()
    finally:
        pictures.close()
    game.sync_to_host()                                          # pull_params
    t7.save_checkpoint(str(tmp_path / "mirror.net"), G=G, D=D)
    game.close()
    ck = t7.load_checkpoint(str(tmp_path / "mirror.net"))
    hG, hD = ck["G"].evaluate(), ck["D"].evaluate()
    images = nn_utils.forwardBatched(hG, vis, B)
    clone = images.copy()
    clone[98], clone[99] = TRAIN_DATA[0], progress.sanity_image(dims, seed, epoch)
    assert np.array_equal(ranked[98], TRAIN_DATA[0]) and np.array_equal(ranked[99], clone[99]) and np.array_equal(ranked, clone)
    preds = nn_utils.forwardBatched(hD, clone, B).reshape(100, -1)[:, 0]
    assert np.array_equal(out["predictions"].view(np.uint32), preds.view(np.uint32))
    good, bad = nn_utils.predictionOrder(preds, False, 50), nn_utils.predictionOrder(preds, True, 50)
    assert np.array_equal(out["good"], good) and np.array_equal(out["bad"], bad) and len(good) == len(bad) == 50
    fs = progress.space_of(colorSpace)
    to_rgb = lambda t: ctx.colorspace(t, fs, L.GR_CS_RGB)          # y or yuv
    for kind, table, rows, gh, gw in (("images", images, np.arange(100), 10, 10), ("images_good", clone, good, 7, 7),
                                      ("images_bad", clone, bad, 7, 7), ("images_train", TRAIN_DATA[:50], np.arange(50), 8, 7)):
        want = po.quantise(po.progress_grid(table, rows, len(rows), gh, gw, epoch, fs, to_rgb))
        assert np.array_equal(out["u8"][kind], want), kind
        assert png_size(out["paths"][kind]) == want.shape[:2] and out["paths"][kind] == progress.epoch_picture_path(str(tmp_path), kind, 7, epoch)


def test_a_continued_run_shows_the_same_faces(ctx, tmp_path):
    """--network with --progress reuses the checkpoint's vis_noise_inputs (train.lua:116): the first picture of the continued run, drawn
    from the loaded weights before any batch, is G(vis_noise_inputs) of the checkpoint - all 100 cells of images/, the first 98 included"""
    from ganrev import nn_utils, png, progress, t7, train
    args = SMALL + ["--epochs", "1", "--N_epoch", "2", "--colorSpace", "gray", "--progress"]
    first = train.main(args + ["--save", str(tmp_path / "a")])
    second = train.main(args + ["--save", str(tmp_path / "b"), "--network", first["path"], "--seed", "9"])      # another seed: fresh noise would differ
    assert second["epoch"] == 2 and np.array_equal(second["pictures"].vis_noise_inputs, first["pictures"].vis_noise_inputs)
    assert [r[0] for r in second["pictures"].plot_data] == [1, 2]
    ck = t7.load_checkpoint(first["path"])
    images = nn_utils.forwardBatched(ck["G"].evaluate(), ck["vis_noise_inputs"], 4)
    want = po.quantise(po.progress_grid(images, np.arange(100), 100, 10, 10, 2, 1, lambda t: np.repeat(t, 3, axis=1)))
    got = np.asarray(png.read_png(progress.epoch_picture_path(str(tmp_path / "b"), "images", second["pictures"].start, 2)))
    assert np.array_equal(got.reshape(want.shape), want)
