"""What the script modules (train, train_r, pretrain_g, pretrain_with_previous_net, sample) say the same way: image geometry from a
colour-space name, the CxHxW_ndN part of their checkpoint names, a checkpoint's opt table, loading a checkpoint for good, and the
--dataset / --fileExtension options with the DATASET.* calls every reference script opens with."""
from . import _lib as L
from . import t7


def image_dims(colorSpace, height, width):
    """(channels, height, width): one channel for y (train.lua:45) or gray (ganrev.train's name for it), else three"""
    return (1 if colorSpace in ("y", "gray") else 3, int(height), int(width))


def needs_conversion(images, colorSpace):
    """three-channel (rgb) images that --colorSpace y | yuv | hsl asks to see in another space (dataset.lua:153)"""
    return colorSpace in ("y", "yuv", "hsl") and images.shape[1] == 3


def geometry(dims, noiseDim):
    """CHANNELSxHEIGHTxWIDTH_ndNOISEDIM, as every reference script names its checkpoint (train.lua:148, train_r.lua:231)"""
    return "%dx%dx%d_nd%d" % (dims[0], dims[1], dims[2], noiseDim)


def opt_table(OPT):
    """The scalar options, in the order the parser declares them, as a checkpoint's `opt` (train.lua:256 saves OPT itself).
    dataset and fileExtension are saved only when --dataset names a directory: a run that reads no folder writes the checkpoint it
    wrote before these options existed, byte for byte."""
    skip = ("dataset", "fileExtension") if getattr(OPT, "dataset", "NONE") == "NONE" else ()
    return {k.rstrip("_"): v for k, v in vars(OPT).items() if isinstance(v, (int, float, str, bool)) and k not in skip}      # continue_ -> continue


def load_checkpoint(path):
    """t7.load_checkpoint, or an error when the file holds classes this package cannot convert"""
    ck = t7.load_checkpoint(path)
    if "_unconverted" in ck:
        raise L.GanrevError(f"{path}: {ck['_unconverted']}")
    return ck


# ---------------------------------------------------------------------------------------------------------------------
# The dataset loader (ganrev.dataset = dataset.lua).  Every reference script has `--dataset` (default "NONE") and opens with
#   DATASET.setColorSpace(OPT.colorSpace); DATASET.setFileExtension("jpg"); DATASET.setHeight(..); DATASET.setWidth(..); DATASET.setDirs({OPT.dataset})
# (train.lua:81-85, train_r.lua:93-97, apply_r.lua:83-87, sample.lua:46-50, pretrain_g.lua:60-64, pretrain_with_previous_net.lua:69-73).
def add_dataset_options(p):
    p.add_argument("--dataset", default="NONE", help="directory of image files to load with ganrev.dataset (dataset.lua); NONE: --data or synthetic images")
    p.add_argument("--fileExtension", default="jpg", help="only files whose name ends in this are loaded (the reference hard-codes jpg)")
    # True when given, None (not False) when absent, like --progress: a run without it saves the opt table it saved before the option existed
    p.add_argument("--cacheDataset", action="store_true", default=None,
                   help="decode every file of --dataset once and keep the bytes on the GPU: each draw is then one launch, same images bit for bit "
                        "(needs --dataset and the device-resident loop; apply_r and train_r configure the dataset and - but for apply_r --needles / --real - never read it: they accept and ignore this)")


def add_progress_option(p):
    """--progress: True when given, None (not False) when absent - opt_table saves scalars, so a run without the option writes the opt table,
    and with it the checkpoint, it wrote before the option existed"""
    p.add_argument("--progress", action="store_true", default=None,
                   help="write the reference's visualizeProgress pictures and plot_data.json under --save (ganrev.progress); off: nothing changes")


def refuse_progress_in_compat(OPT):
    """--progress draws from the device-resident loop's nets where they lie (ganrev.progress); the --compat loops keep their parameters in
    host vectors that every forward uploads, so they have no such state to look at: the combination is refused, not approximated."""
    if OPT.progress and OPT.compat:
        raise L.GanrevError("--progress needs the device-resident loop: it cannot be combined with --compat")


def open_dataset(OPT, colorSpace, height, width, ctx=None, reads=True):
    """The five DATASET.set* calls of a script's head when --dataset names a directory -> the configured ganrev.dataset module, else None.
    The reference asserts OPT.dataset ~= "NONE"; here NONE keeps --data / the synthetic images.  Giving both --data and --dataset is an error.
    The permutations of loadRandomImages are seeded from --seed.  --cacheDataset: DATASET.cache(ctx) before the first draw (an error without
    --dataset, and with --compat, whose host loops have no use for a device table); reads=False (train_r, and apply_r without
    --needles / --real: the dataset is configured, never read) ignores it."""
    want_cache = bool(getattr(OPT, "cacheDataset", None)) and reads
    if want_cache and OPT.dataset == "NONE":
        raise L.GanrevError("--cacheDataset needs --dataset: there are no files to keep")
    if want_cache and getattr(OPT, "compat", False):
        raise L.GanrevError("--cacheDataset needs the device-resident loop: it cannot be combined with --compat")
    if OPT.dataset == "NONE":
        return None
    if getattr(OPT, "data", ""):
        raise L.GanrevError("--data and --dataset both given: the images come from one of them")
    from . import dataset as DATASET
    DATASET.setColorSpace("y" if colorSpace == "gray" else colorSpace)
    DATASET.setFileExtension(OPT.fileExtension)
    DATASET.setHeight(height)
    DATASET.setWidth(width)
    DATASET.setDirs([OPT.dataset])
    DATASET.setSeed(getattr(OPT, "seed", 0))
    if want_cache:
        DATASET.cache(ctx, quiet=getattr(OPT, "quiet", True))
    return DATASET


def load_random_images(DATASET, count):
    """DATASET.loadRandomImages(count) as the training loops take it (train.lua:216, pretrain_g.lua:118, pretrain_with_previous_net.lua:171): a
    host array, or with a live cache the device table (nn_utils.DeviceTensor) where the one launch left it - the caller frees it.  A folder
    with fewer files than the loop will index is an error here, not an index past the end there"""
    res = DATASET.loadRandomImages(count, device=DATASET.cached())
    if res.size() < count:
        res.free()
        raise L.GanrevError(f"--dataset holds {res.size()} matching files, the loop needs {count}")
    return res.images
