"""numpy restatement of gr_progress_grid_dev (include/ganrev.h states the layout): zero-fill the grid, place the tiles, draw the epoch's
digits at the stated coordinates.  The colour step is a callable the caller hands in (the GPU tests pass gr_colorspace_host); nothing
here imports the product package.  tests/test_progress_host.py pins this file against a hand-written array.
"""
import numpy as np

import imagegrid_oracle as io_

F = np.float32

# the ten digits as 3 x 5 blocks, "#" = 1: seven-segment shapes; "1" is the right-hand column only, the middle bar of "3" is two pixels
GLYPHS = [np.array([[ch == "#" for ch in row] for row in g.split()], F) for g in (
    "### #.# #.# #.# ###", "..# ..# ..# ..# ..#", "### ..# ### #.. ###", "### ..# .## ..# ###", "#.# #.# ### ..# ..#",
    "### #.. ### ..# ###", "### #.. ### #.# ###", "### ..# ..# ..# ..#", "### #.# ### #.# ###", "### #.# ### ..# ###")]


def shape(channels, h, w, from_space, grid_h, grid_w):
    return (3 if from_space >= 0 else channels, grid_h * h + 7, grid_w * w)


def progress_grid(table, rows, n_show, grid_h, grid_w, epoch, from_space=-1, to_rgb=None):
    """-> float32 [Cout x GH x GW].  to_rgb(images [n x C x h x w]) -> [n x 3 x h x w]: asked for when from_space >= 0."""
    table = np.asarray(table, F)
    _, c, h, w = table.shape
    cout, gh, gw = shape(c, h, w, from_space, grid_h, grid_w)
    grid = np.zeros((cout, gh, gw), F)
    for t in range(min(n_show, grid_h * grid_w)):
        tile = table[int(rows[t])][None]
        if from_space >= 0:
            tile = np.asarray(to_rgb(tile), F)
        y0, x0 = (t // grid_w) * h, (t % grid_w) * w
        grid[:, y0:y0 + h, x0:x0 + w] = tile[0]
    for p, ch in enumerate(reversed(str(int(epoch))), start=1):         # least significant digit first
        grid[:, gh - 7:gh - 2, gw - 2 - 6 * p:gw - 6 * p + 1] = GLYPHS[int(ch)]
    return grid


def quantise(grid):
    """uint8 [GH x GW x Cout] by gr_image_grid_dev's rule with lo = 0, hi = 1: clamp by compare-selects, then min(255, max(0, trunc(v * 255 + 0.5)))"""
    with np.errstate(all="ignore"):
        g = np.asarray(grid, F)
        g = np.where(g < F(0), F(0), g)
        g = np.where(g > F(1), F(1), g)
    return io_.quantise(g)
