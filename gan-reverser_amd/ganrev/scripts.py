"""What the script modules (train, train_r, pretrain_g, pretrain_with_previous_net, sample) say the same way: image geometry from a
colour-space name, the CxHxW_ndN part of their checkpoint names, a checkpoint's opt table and loading a checkpoint for good."""
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
    """The scalar options, in the order the parser declares them, as a checkpoint's `opt` (train.lua:256 saves OPT itself)."""
    return {k.rstrip("_"): v for k, v in vars(OPT).items() if isinstance(v, (int, float, str, bool))}      # continue_ -> continue


def load_checkpoint(path):
    """t7.load_checkpoint, or an error when the file holds classes this package cannot convert"""
    ck = t7.load_checkpoint(path)
    if "_unconverted" in ck:
        raise L.GanrevError(f"{path}: {ck['_unconverted']}")
    return ck
