"""The pictures apply_r.lua and sample.lua end in, rendered on the GPU from device-resident image tables (gr_image_grid_dev).

Every product is image.toDisplayTensor over a gathered list of rows plus the reference's decorations; each function below names the
reference lines it mirrors, takes DeviceTensors [N x C x H x W] and row indices, returns the picture as a uint8 array [GH x GW x 1|3]
and, given `path`, writes it as PNG (ganrev.png).  The reference writes JPEG (image.save); JPEG is lossy, so no byte parity with its
files is claimed: the 8-bit quantisation here is u8 = min(255, trunc(v * 255 + 0.5)) of the display value v (include/ganrev.h).

image.toDisplayTensor fills the cells no image covers with the maximum of its (normalised) input - 1.0 as soon as one pixel
saturates.  Here that filler is the argument `fill`, 1.0 by default.  (`image` is an un-vendored rock: DESIGN.md section 1.)

from_space is a colour-space name ("rgb", "y", "yuv", "hsl": the images go through NN_UTILS.toRgb first) or None (channels as they
are; a 1-channel table then gives a 1-channel picture).
"""
import math

import numpy as np

from . import _lib as L
from . import png
from .nn_utils import DeviceTensor

BLUE, RED, BLACK = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)


def _space(from_space):
    if from_space is None:
        return -1
    if from_space not in L.COLOR_SPACES:
        raise ValueError(f"Unknown color space <from>: '{from_space}'")          # utils/nn_utils.lua:165
    return L.COLOR_SPACES[from_space]


def grid(images_dev, rows, nrow, from_space="rgb", padding=0, margin=0, bg=None, inset=None, inset_rgb=BLUE, fill=1.0,
         lo=0.0, hi=1.0, auto_range=False, path=None, want_float=False):
    """image.toDisplayTensor{input = images[rows], nrow = nrow, min = lo, max = hi} (auto_range: without min / max) in one launch (two
    with auto_range).  images_dev: one DeviceTensor, or a tuple of two for tiles of two images side by side (rows is then [n x 2]); a row
    of -1 leaves the tile's background bg[t] (default black), which also paints the `margin` ring around the tile.
    -> uint8 [GH x GW x Cout]; with want_float (uint8, float32 [Cout x GH x GW])."""
    tabs = tuple(images_dev) if isinstance(images_dev, (tuple, list)) else (images_dev,)
    ctx = tabs[0].ctx
    _, c, h, w = tabs[0].shape
    for t in tabs[1:]:
        if tuple(t.shape[1:]) != (c, h, w):
            raise ValueError(f"tables of one grid hold images of one shape: {tabs[0].shape[1:]} and {t.shape[1:]}")
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(tabs))
    fs = _space(from_space)
    cout, gh, gw = L.grid_shape(len(rows), len(tabs), c, h, w, fs, nrow, padding, margin)
    u8_dev = ctx.malloc(cout * gh * gw)
    f_dev = ctx.malloc(4 * cout * gh * gw) if want_float else None
    try:
        ctx.image_grid_dev([t.ptr for t in tabs], [t.shape[0] for t in tabs], c, h, w, fs, rows, nrow, padding, margin, bg, inset,
                           inset_rgb if inset is not None else None, fill, auto_range, lo, hi, f_dev, u8_dev)
        u8 = ctx.download(u8_dev, (gh, gw, cout), np.uint8)
        f = ctx.download(f_dev, (cout, gh, gw), np.float32) if want_float else None
    finally:
        ctx.free(u8_dev)
        if f_dev is not None:
            ctx.free(f_dev)
    if path:
        png.write_png(path, u8)
    return (u8, f) if want_float else u8


def variations_grid(images_dev, nbSteps=16, from_space=None, path=None):
    """apply_r.lua:136-138: every image of the table, one noise component per row of nbSteps.  The reference hands G's output to
    toDisplayTensor without toRgb; from_space = None keeps that."""
    return grid(images_dev, np.arange(images_dev.shape[0]), nbSteps, from_space, path=path)


def cluster_grid(images_dev, rows, from_space="rgb", face_dev=None, path=None):
    """apply_r.lua:245-258: the cluster's average face, then its images (`rows`, in the cluster's order); nrow = ceil(sqrt(1 + n)).
    face_dev: the average face as a DeviceTensor [C x H x W] (createClusterImagesDev has it); computed here (gr_rows_mean_dev) when None."""
    ctx = images_dev.ctx
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n, d = len(rows), images_dev.size // images_dev.shape[0]
    sheet = DeviceTensor(ctx, (1 + n,) + tuple(images_dev.shape[1:]))               # tnsr of :250-254: one table for the grid to gather from
    try:
        if face_dev is None:
            ctx.rows_mean_dev(images_dev.ptr, images_dev.shape[0], d, rows, sheet.ptr)
        else:
            ctx.copy2d(sheet.ptr, d, face_dev.ptr, d, 1, d)
        for j, r in enumerate(rows):
            ctx.copy2d(sheet.ptr + 4 * d * (1 + j), d, images_dev.ptr + 4 * d * int(r), d, 1, d)
        return grid(sheet, np.arange(1 + n), math.ceil(math.sqrt(1 + n)), from_space, path=path)
    finally:
        sheet.free()


def similar_grid(images_dev, rows, from_space="rgb", path=None):
    """apply_r.lua:278-298: the needle's most similar rows, best first (the needle itself leads), nrow = ceil(sqrt(n)); the blue frame
    of :286-295 is drawn over the first image's own edge pixels."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    inset = np.zeros(len(rows), np.uint8)
    inset[0] = 1
    return grid(images_dev, rows, math.ceil(math.sqrt(len(rows))), from_space, inset=inset, inset_rgb=BLUE, path=path)


def similar_example_grid(needle_images_dev, needle_row, images_dev, rows, from_space="rgb", path=None):
    """similar_grid for a search by example: the needle image - row `needle_row` of ITS table, it is no row of the corpus - in the first cell
    with the blue frame, then the hits `rows` of the corpus table, best first; nrow = ceil(sqrt(1 + n)).  The 1 + n images are gathered
    into one sheet on the device (as cluster_grid does with the average face) and drawn by the same launch."""
    ctx = images_dev.ctx
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    n, d = len(rows), images_dev.size // images_dev.shape[0]
    if tuple(needle_images_dev.shape[1:]) != tuple(images_dev.shape[1:]):
        raise ValueError(f"needle images {needle_images_dev.shape[1:]} and corpus images {images_dev.shape[1:]} differ in shape")
    sheet = DeviceTensor(ctx, (1 + n,) + tuple(images_dev.shape[1:]))
    try:
        ctx.copy2d(sheet.ptr, d, needle_images_dev.ptr + 4 * d * int(needle_row), d, 1, d)
        for j, r in enumerate(rows):
            ctx.copy2d(sheet.ptr + 4 * d * (1 + j), d, images_dev.ptr + 4 * d * int(r), d, 1, d)
        inset = np.zeros(1 + n, np.uint8)
        inset[0] = 1
        return grid(sheet, np.arange(1 + n), math.ceil(math.sqrt(1 + n)), from_space, inset=inset, inset_rgb=BLUE, path=path)
    finally:
        sheet.free()


def fixed_pairs_grid(images_dev, fixed_dev, nbPairs, from_space="rgb", path=None):
    """apply_r.lua:325-342: image i and its fixed version side by side on a blue field with a 1-pixel border, 4 pairs per row"""
    i = np.arange(nbPairs, dtype=np.int64)
    return grid((images_dev, fixed_dev), np.stack([i, i], axis=1), 4, from_space, margin=1, bg=np.tile(np.float32(BLUE), (nbPairs, 1)), path=path)


def fixed_images_grid(images_dev, n, path=None):
    """apply_r.lua:345-351: the first n images, nrow = floor(sqrt(n)).  The reference skips toRgb here (fixed and unfixed sheet alike):
    the channels are shown as they are, whatever the colour space."""
    return grid(images_dev, np.arange(n), int(math.floor(math.sqrt(n))), None, path=path)


def anomalies_grid(images_dev, is_anomaly, from_space="rgb", path=None):
    """apply_r.lua:374-389: the first len(is_anomaly) images, each with a 1-pixel frame - red (channel 1 of the whole tile set to 1, then
    the interior overwritten) around an anomaly, black around the others; nrow = floor(sqrt(n))."""
    flag = np.asarray(is_anomaly, dtype=bool).reshape(-1)
    n = len(flag)
    bg = np.where(flag[:, None], np.float32(RED), np.float32(BLACK)).astype(np.float32)
    return grid(images_dev, np.arange(n), int(math.floor(math.sqrt(n))), from_space, margin=1, bg=bg, path=path)


def neighbours_grid(images_dev, rows, table_dev, neighbour_rows, from_space="rgb", path=None):
    """sample.lua:173-185 toNeighboursGrid: image, neighbour, image, neighbour, ... with nrow = the number of pairs, no min / max (auto
    range).  Rendered as tiles of two images, pairs / 2 tiles per row: the same pixels for an even number of pairs (16 in sample.lua:114);
    an odd number would split a pair over two rows and is refused."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    nb = np.asarray(neighbour_rows, dtype=np.int64).reshape(-1)
    if len(rows) != len(nb) or len(rows) % 2:
        raise ValueError(f"neighbours_grid: an even number of (image, neighbour) pairs, not {len(rows)} and {len(nb)}")
    return grid((images_dev, table_dev), np.stack([rows, nb], axis=1), len(rows) // 2, from_space, auto_range=True, path=path)


# the ring colours of map_grid: cluster label j takes MAP_PALETTE[j % 12] (twelve hues at full saturation, ordered so that neighbours in the
# list are far apart on the colour wheel); a tile without a label, and an empty cell, keep MAP_FIELD
MAP_PALETTE = ((1.0, 0.0, 0.0), (0.0, 0.5, 1.0), (0.0, 0.8, 0.0), (1.0, 0.5, 0.0), (0.5, 0.0, 1.0), (0.0, 0.8, 0.8),
               (1.0, 0.0, 0.5), (0.5, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.8, 0.0), (1.0, 0.0, 1.0), (0.0, 1.0, 0.5))
MAP_FIELD = (0.0, 0.0, 0.0)


def map_colours(cell_rows, labels=None):
    """bg [cells x 3] of map_grid: MAP_PALETTE[label % 12] for a cell that shows a row with a label >= 0, MAP_FIELD for the others"""
    rows = np.asarray(cell_rows, dtype=np.int64).reshape(-1)
    bg = np.tile(np.float32(MAP_FIELD), (len(rows), 1))
    if labels is not None:
        labels = np.asarray(labels, dtype=np.int64).reshape(-1)
        shown = rows >= 0
        lab = labels[rows[shown]]
        colours = np.float32(MAP_PALETTE)[lab % len(MAP_PALETTE)]
        colours[lab < 0] = np.float32(MAP_FIELD)
        bg[shown] = colours
    return bg


def map_grid(images_dev, cell_rows, from_space="rgb", labels=None, path=None):
    """The faces drawn where they land on a two-dimensional map (ganrev.tsne.mapCells): cell_rows [grid_h x grid_w] holds the row shown in each
    cell, -1 for an empty one, which stays MAP_FIELD.  One launch; every tile has a 1-pixel ring, coloured by labels[row] (the cluster of the
    row: map_colours) when labels are given."""
    cell_rows = np.asarray(cell_rows, dtype=np.int64)
    return grid(images_dev, cell_rows.reshape(-1), cell_rows.shape[1], from_space, margin=1, bg=map_colours(cell_rows, labels), path=path)
