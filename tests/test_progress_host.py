"""not-gpu: the host side of the trainers' progress pictures (ganrev.progress) - the --progress option of the four scripts, the file
names, the plot_data.json schema - and the numpy grid the GPU tests compare gr_progress_grid_dev with (tests/progress_oracle.py),
pinned here against an array written out by hand."""
import json
import os

import numpy as np
import pytest

import progress_oracle as po

SCRIPTS = ("train", "train_r", "pretrain_g", "pretrain_with_previous_net")


@pytest.mark.parametrize("script", SCRIPTS)
def test_progress_option_is_off_by_default(script):
    import importlib
    mod = importlib.import_module("ganrev." + script)
    assert not mod.parse([]).progress
    assert mod.parse(["--progress"]).progress is True


@pytest.mark.parametrize("script", SCRIPTS)
def test_checkpoint_opt_table_names_progress_only_when_it_is_given(script):
    """without --progress a run writes the opt table it wrote before the option existed"""
    import importlib
    from ganrev import scripts
    mod = importlib.import_module("ganrev." + script)
    assert "progress" not in scripts.opt_table(mod.parse([]))
    assert scripts.opt_table(mod.parse(["--progress"]))["progress"] is True


@pytest.mark.parametrize("script", SCRIPTS)
def test_compat_loops_refuse_progress(script):
    """refused before anything touches the GPU"""
    import importlib
    import ganrev._lib as L
    mod = importlib.import_module("ganrev." + script)
    with pytest.raises(L.GanrevError, match="--compat"):
        mod.main(["--progress", "--compat"])


def test_file_name_patterns():
    from ganrev import progress
    assert progress.epoch_picture_path("logs", "images", 1700000000, 3) == os.path.join("logs", "images", "1700000000_00003.png")
    assert progress.epoch_picture_path("out", "images_good", 5, 12345) == os.path.join("out", "images_good", "5_12345.png")
    assert progress.progress_path("logs", "pairs", 25) == os.path.join("logs", "progress", "pairs_00025.png")
    assert progress.progress_path("logs", "decoded", 2) == os.path.join("logs", "progress", "decoded_00002.png")
    assert progress.plot_data_path("logs") == os.path.join("logs", "plot_data.json")


@pytest.mark.parametrize("script, row", [("train", [1, 0.7, 0.6]), ("pretrain_g", [2, 0.01]), ("train_r", [100, 0.1, 0.2, 0.4])])
def test_plot_data_json_schema(tmp_path, script, row):
    from ganrev import progress
    path = progress.write_plot_data(str(tmp_path), script, [row, row])
    assert path == os.path.join(str(tmp_path), "plot_data.json")
    doc = json.load(open(path))
    assert sorted(doc) == ["data", "labels", "script"]
    assert doc["script"] == script and doc["labels"] == progress.PLOT_LABELS[script]
    assert doc["data"] == [[float(v) for v in row]] * 2 and len(doc["labels"]) == len(row)
    with pytest.raises(ValueError):
        progress.write_plot_data(str(tmp_path), script, [row + [1.0]])


def test_train_r_plot_row_is_low_avg_high_of_the_last_hundred_losses():
    from ganrev import progress
    losses = [9.0] * 7 + [float(v) for v in range(1, 101)]
    assert progress.loss_window_row(200, losses) == [200, 1.0, 50.5, 100.0]


def test_sanity_image_is_the_references():
    """train.lua:275-285: uniform(0, 0.5); channel 0 (only) carries the diagonal of 1.0 and 0.5 at every fourth crossing off it"""
    from ganrev import progress, synth
    img = progress.sanity_image((3, 8, 8), 1, 2)
    base = synth.uniform((3, 8, 8), progress.sanity_seed(1, 2), 0.0, 0.5)
    assert img.dtype == np.float32 and np.array_equal(img[1:], base[1:]) and base.min() >= 0 and base.max() <= 0.5
    for i in range(8):
        for j in range(8):
            want = 1.0 if i == j else 0.5 if (i + 1) % 4 == 0 and (j + 1) % 4 == 0 else base[0, i, j]
            assert img[0, i, j] == np.float32(want), (i, j)


def test_the_numpy_grid_against_a_hand_written_array():
    """a 1 x 1 grid of one 1 x 2 x 20 tile at epoch 42: GH x GW = 9 x 20; "2" (digit 1) in columns 12..14, "4" (digit 2) in columns 6..8,
    both in rows 2..6; the tile above them, two zero rows below"""
    tile = (np.arange(40, dtype=np.float32).reshape(1, 1, 2, 20) - 4) / 32          # -0.125 .. 1.09375: below 0 and above 1
    digits = ["......#.#...###.....",
              "......#.#.....#.....",
              "......###...###.....",
              "........#...#.......",
              "........#...###....."]
    want = np.zeros((1, 9, 20), np.float32)
    want[0, 0:2] = tile[0, 0]
    want[0, 2:7] = [[ch == "#" for ch in row] for row in digits]
    got = po.progress_grid(np.concatenate([tile * 0 + 7, tile]), [1], 1, 1, 1, 42)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    u8 = po.quantise(got)
    assert u8.shape == (9, 20, 1) and u8.dtype == np.uint8
    assert u8[0, 0, 0] == 0 and u8[0, 4, 0] == 0 and u8[0, 5, 0] == 8 and u8[1, 16, 0] == 255 and u8[1, 19, 0] == 255      # clamp at both ends
    assert np.array_equal(u8[2:7, :, 0], want[0, 2:7].astype(np.uint8) * 255) and not u8[7:].any()
    # an empty grid keeps only the digits; rows beyond the grid are ignored
    assert np.array_equal(po.progress_grid(tile, [0], 0, 1, 1, 42)[0, 2:], want[0, 2:]) and not po.progress_grid(tile, [0], 0, 1, 1, 42)[0, :2].any()
    assert np.array_equal(po.progress_grid(tile, [0, 0, 0], 3, 1, 1, 42), po.progress_grid(tile, [0], 1, 1, 1, 42))
