"""not-gpu: the --cacheDataset option in the six scripts (parsed, saved only when given, refused where it has nothing to work on), the new
entry points in the header, the cdef and the bindings, and ganrev.dataset.cache() on a machine without a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["gr_dataset_cache_create", "gr_dataset_cache_destroy", "gr_dataset_cache_append", "gr_dataset_cache_size", "gr_dataset_cache_image",
                "gr_dataset_cache_load_dev"]
SCRIPTS = ["train", "train_r", "apply_r", "sample", "pretrain_g", "pretrain_with_previous_net"]


def parse(script, argv):
    import importlib
    return importlib.import_module("ganrev." + script).parse(argv)


@pytest.mark.parametrize("script", SCRIPTS)
def test_the_option_parses_in_every_script_and_is_saved_only_when_given(script):
    from ganrev import scripts
    absent = parse(script, [])
    given = parse(script, ["--dataset", "faces", "--cacheDataset"])
    assert absent.cacheDataset is None and given.cacheDataset is True
    assert "cacheDataset" not in scripts.opt_table(absent)
    assert scripts.opt_table(given)["cacheDataset"] is True
    # a run without the option saves the table it saved before the option existed: the same keys as a namespace that never had it
    before = parse(script, [])
    del before.cacheDataset
    assert scripts.opt_table(absent) == scripts.opt_table(before)
    with_folder, before = parse(script, ["--dataset", "faces"]), parse(script, ["--dataset", "faces"])
    del before.cacheDataset
    assert list(scripts.opt_table(with_folder).items()) == list(scripts.opt_table(before).items())


def test_the_option_is_refused_without_a_dataset_and_in_compat_mode(tmp_path):
    from ganrev import scripts
    from ganrev._lib import GanrevError
    with pytest.raises(GanrevError, match="needs --dataset"):
        scripts.open_dataset(parse("train", ["--cacheDataset"]), "rgb", 16, 16)
    for script in ("train", "pretrain_g", "pretrain_with_previous_net"):
        with pytest.raises(GanrevError, match="--compat"):
            scripts.open_dataset(parse(script, ["--dataset", str(tmp_path), "--cacheDataset", "--compat"]), "rgb", 16, 16)
    # apply_r and train_r configure the dataset and never read it: they accept the option and ignore it (no cache, no device needed)
    from ganrev import dataset
    saved = {k: getattr(dataset, k) for k in ("dirs", "fileExtension", "height", "width", "colorSpace", "paths", "_seed", "_draws")}
    try:
        for script in ("apply_r", "train_r"):
            assert scripts.open_dataset(parse(script, ["--dataset", str(tmp_path), "--cacheDataset"]), "rgb", 16, 16, reads=False) is dataset
            assert not dataset.cached()
        assert scripts.open_dataset(parse("train_r", ["--cacheDataset"]), "rgb", 16, 16, reads=False) is None
    finally:
        for k, v in saved.items():
            setattr(dataset, k, v)
    for script in ("apply_r", "train_r"):
        import importlib
        src = open(importlib.import_module("ganrev." + script).__file__).read()
        assert re.search(r"open_dataset\([^\n]*reads=False", src), script


def test_the_help_text_says_who_ignores_the_option():
    import argparse
    from ganrev import scripts
    p = argparse.ArgumentParser()
    scripts.add_dataset_options(p)
    text = " ".join(p.format_help().split())
    assert "--cacheDataset" in text and "apply_r and train_r" in text and "ignore" in text


def test_the_header_the_cdef_and_the_bindings_name_the_entry_points():
    import ganrev._lib as L
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    header = strip(open(os.path.join(ROOT, "include", "ganrev.h")).read())
    lua = open(os.path.join(ROOT, "gan-reverser_amd", "lua", "hipnn.lua")).read()
    cdef = strip(re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1))
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/ganrev.h"
        assert re.search(r"\bint\s+%s\s*\(" % name, cdef), f"{name} is not declared in hipnn.lua's cdef"
        assert name in L.EXPORTED_SYMBOLS and name in L._SIGS
    for method in ("append", "size", "image", "load_dev", "close"):
        assert callable(getattr(L.DatasetCache, method))


def test_a_dropped_cache_is_destroyed_while_its_context_is_open_and_left_alone_after():
    """the rule of the nets (tests/test_net_lifetime_host.py), on a stub library that records the calls"""
    import gc
    import ganrev._lib as L

    class Lib:
        destroyed = []

        def gr_dataset_cache_destroy(self, h):
            self.destroyed.append(h)
            return 0

    class Ctx:
        def __init__(self, lib, h):
            self.lib, self.h = lib, h

    def cache(ctx, h):
        c = object.__new__(L.DatasetCache)
        c.ctx, c.lib, c.h = ctx, ctx.lib, h
        return c
    lib = Lib()
    c = cache(Ctx(lib, 1234), 5)
    del c
    gc.collect()
    assert lib.destroyed == [5]
    c = cache(Ctx(lib, None), 6)                                              # its context was shut down
    del c
    gc.collect()
    assert lib.destroyed == [5]
    c = cache(Ctx(lib, 1234), 7)
    c.close(); c.close()
    del c
    gc.collect()
    assert lib.destroyed == [5, 7]


def test_cache_without_a_device_raises_and_leaves_the_module_usable(tmp_path):
    import numpy as np
    import torch
    from ganrev import dataset, png
    from ganrev._lib import GanrevError
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    saved = {k: getattr(dataset, k) for k in ("dirs", "fileExtension", "height", "width", "colorSpace", "paths", "_seed", "_draws")}
    try:
        for i in range(3):
            png.write_png(str(tmp_path / ("f%d.png" % i)), np.full((4, 5, 3), 40 * i, np.uint8))
        dataset.setDirs([str(tmp_path)]); dataset.setFileExtension("png")
        with pytest.raises(GanrevError):
            dataset.cache()
        assert not dataset.cached()
        assert [os.path.basename(f) for f in dataset.loadPaths()] == ["f0.png", "f1.png", "f2.png"]
        assert dataset.randomIndices(2, seed=1).shape == (2,) and dataset.imageIndices(2, 5).tolist() == [1, 2]
        assert dataset.decode(dataset.paths[1]).shape == (4, 5, 3)
        dataset.uncache()                                                     # nothing to release: no error
    finally:
        for k, v in saved.items():
            setattr(dataset, k, v)
