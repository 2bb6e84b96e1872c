"""Mirror of the reference's dataset.lua, name for name: a folder of image files becomes the [N x C x H x W] float tensor every
script starts from (train.lua:81-85,216; train_r.lua:93-97; apply_r.lua:83-87; sample.lua:46-50,77,132; pretrain_g.lua:60-64,105,118,225;
pretrain_with_previous_net.lua:69-73,144,171,279).

    from ganrev import dataset as DATASET
    DATASET.setColorSpace("yuv"); DATASET.setFileExtension("jpg"); DATASET.setHeight(32); DATASET.setWidth(32)
    DATASET.setDirs(["faces/"])
    TRAIN_DATA = DATASET.loadRandomImages(10000)        # .images / .data: a nn_utils.DeviceTensor [N x 3 x 32 x 32]; .indices; .size()

Per file the reference runs image.load -> image.scale -> (per tensor) rgbToColorSpace [-> NN_UTILS.normalize].  Here the host only
DECODES a file to the bytes it stores (uint8, interleaved HWC, 1 / 3 / 4 channels); files of equal source size are uploaded together
as bytes and one gr_dataset_images_dev launch per chunk does the rest on the GPU (include/ganrev.h states the arithmetic).  The fp32
image at source size never exists on the host.  A folder of mixed sizes is processed in groups of equal size; each group's images
are then moved to their places in the result on the device.

DATASET.cache() (the scripts' --cacheDataset) decodes every file ONCE and keeps the bytes on the device as the files store them
(_lib.DatasetCache); from then on loadImages / loadRandomImages draw the indices they always drew and make one
gr_dataset_cache_load_dev launch over the drawn images, whatever sizes they mix - the same bits, no decoding, no upload.  The cache holds
source bytes, so setHeight / setWidth / setColorSpace / setNbChannels keep it; setDirs and setFileExtension change the files and drop it.

Decoders: .png through ganrev.png (8-bit grey / RGB / RGBA); .npy holding uint8 [H x W] or [H x W x 1|3|4] as it is; everything else
(the reference's jpg) through Pillow when it can be imported.  Without Pillow such a file raises GanrevError naming the file and the
missing decoder - pixels are never guessed.

Deviations from dataset.lua, each on purpose:
  :142      torch.randperm draws from Torch's global generator, which is not reproduced.  The permutation is
            numpy.random.Generator(PCG64(seed)).permutation(#paths): seed = the `seed` argument, or (setSeed's seed, number of draws so
            far).  The drawn file indices (0-based, into .paths) are exposed as result.indices.
  :108      loadImages computes N = min(count, #paths) whatever startAt is, and would index past the end of the paths (image.load(nil)).
            Here N = min(count, #paths - startAt + 1): the files that exist from startAt on.
  :100      sample.lua:132 calls loadImages(0, 9999999), which trips dataset.lua's own assert(startAt > 0); ganrev.sample calls it with 1.
  :111      loadImages passes nbChannels to image.load (loadRandomImages passes 3, :149).  nbChannels None (the reference's default: the
            setter is never called) or 3 loads like loadRandomImages.  nbChannels 1 accepts grey files only: image.load's own colour ->
            grey conversion belongs to the `image` rock and is not restated, so a colour file then raises GanrevError.
  :77       `file:find(ext .. '$')` is a Lua pattern; the extension is taken literally here (a plain suffix test, no dot added).
  :162-165  result:normalize() on a device-resident result needs the kernel's normalise step: pass normalize=True to the load call (the
            fused launch then ends in it) - normalize() afterwards returns the dummy (0.5, 0.5).  On a host result (device=False) it is
            nn_utils.normalize, in place.
"""
import importlib
import os

import numpy as np

from . import _lib as L
from . import nn_utils, png

dirs = []
fileExtension = ""
originalHeight = 64          # dataset.lua:13-14: informational there too
originalWidth = 64
height = 32
width = 32
nbChannels = None
colorSpace = "rgb"
paths = None

CHUNK_BYTES = 64 << 20       # decoded bytes of one size uploaded and converted per launch
_seed, _draws = 0, 0
_cache = None                # cache(): the _lib.DatasetCache that holds paths[i] as image i


def setColorSpace(colorSpace_):
    """dataset.lua:27-33"""
    global colorSpace
    assert colorSpace_ in ("rgb", "y", "yuv", "hsl"), colorSpace_
    colorSpace = colorSpace_


def setDirs(dirs_):
    """dataset.lua:37-39.  The cached paths are dropped: the reference keeps paths of the old directories (a second setDirs has no effect there)."""
    global dirs, paths
    dirs = [dirs_] if isinstance(dirs_, (str, bytes, os.PathLike)) else list(dirs_)
    paths = None
    uncache()


def setFileExtension(fileExtension_):
    """dataset.lua:43-45"""
    global fileExtension, paths
    fileExtension = str(fileExtension_)
    paths = None
    uncache()


def setHeight(height_):
    """dataset.lua:49-51"""
    global height
    height = int(height_)


def setWidth(width_):
    """dataset.lua:55-57"""
    global width
    width = int(width_)


def setNbChannels(nbChannels_):
    """dataset.lua:61-63"""
    global nbChannels
    nbChannels = None if nbChannels_ is None else int(nbChannels_)


def setSeed(seed):
    """seed of the permutations loadRandomImages draws when it is given none (module docstring, :142); restarts the draw count"""
    global _seed, _draws
    _seed, _draws = int(seed), 0


def loadPaths():
    """dataset.lua:67-93: every file of every directory whose name ends in the extension, sorted in byte order"""
    global paths
    files = []
    for d in dirs:
        for name in os.listdir(d):                                        # paths.files(dir); "." and ".." never end in an extension
            if name.endswith(fileExtension):
                files.append(os.path.join(d, name))
        files.sort(key=os.fsencode)                                       # table.sort(files, a < b): Lua compares strings by bytes
        if not files:
            raise L.GanrevError("given directory doesnt contain any files of type: " + fileExtension)      # :88
    paths = files
    return paths


def cache(ctx=None, quiet=True):
    """Decode every file of paths once and keep its bytes on the device: image i of the cache is paths[i].  Later loadImages /
    loadRandomImages calls are one launch each (module docstring).  -> the number of files.  A cache that exists is replaced."""
    global _cache
    uncache()
    ctx = ctx or L.default_context()
    if paths is None:
        loadPaths()
    if not quiet:
        print("<dataset> caching %d files" % len(paths))
    held = L.DatasetCache(ctx)
    try:
        for f in paths:
            held.append(decode(f))
    except BaseException:
        held.close()
        raise
    _cache = held
    return len(paths)


def uncache():
    """release the cache (the loads decode their files again)"""
    global _cache
    if _cache is not None:
        held, _cache = _cache, None
        if getattr(held.ctx, "h", None):
            held.close()


def cached():
    """whether loads come from the device-resident cache"""
    return _cache is not None


def imageIndices(startAt, count):
    """0-based file indices loadImages(startAt, count) reads (startAt is 1-based, as in Lua); clamped to the files that exist (:108)"""
    assert startAt > 0                                                    # :100
    assert count > 0                                                      # :101
    if paths is None:
        loadPaths()
    n = max(0, min(int(count), len(paths) - int(startAt) + 1))
    return np.arange(int(startAt) - 1, int(startAt) - 1 + n, dtype=np.int64)


def randomIndices(count, seed=None):
    """0-based file indices loadRandomImages(count) reads: the first min(count, #paths) entries of a seeded permutation (:142-143)"""
    global _draws
    if paths is None:
        loadPaths()
    if seed is None:
        seed = [_seed, _draws]
        _draws += 1
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(len(paths))
    return perm[:max(0, min(int(count), len(paths)))].astype(np.int64)


def decode(path):
    """one file -> uint8 [H x W x 1|3|4] as the file stores it (module docstring: decoders)"""
    low = path.lower()
    if low.endswith(".png"):
        return png.read_png(path)
    if low.endswith(".npy"):
        a = np.load(path, allow_pickle=False)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
            raise L.GanrevError(f"{path}: a .npy image must be uint8 [H x W] or [H x W x 1|3|4], not {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)
    try:
        Image = importlib.import_module("PIL.Image")
    except ImportError:
        raise L.GanrevError(f"{path}: no decoder for this format (ganrev reads .png and uint8 .npy itself; anything else needs Pillow, "
                            "which cannot be imported)") from None
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGB")
        a = np.asarray(im, dtype=np.uint8)
    return np.ascontiguousarray(a[:, :, None] if a.ndim == 2 else a)


class Images:
    """What loadImages / loadRandomImages return (dataset.lua:118-130,155-172): .data / .images [N x C x H x W] (a DeviceTensor, or a host
    array when device=False), size(), len(), indexing, normalize(); plus .indices and .paths (the files, in the order of the rows)."""

    def __init__(self, data, indices, files, normalized):
        self.data = self.images = data
        self.indices, self.paths, self.normalized = indices, files, normalized

    def size(self):
        return len(self.indices)

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        """image i (0-based: Python), [C x H x W]: a host array, or a view of the device tensor"""
        if isinstance(self.data, nn_utils.DeviceTensor):
            i = range(len(self))[i]
            row = self.data.rows(i, i + 1)
            return nn_utils.DeviceTensor(row.ctx, row.shape[1:], row.ptr)
        return self.data[i]

    def normalize(self, mean=None, std=None):
        """dataset.lua:162-165 -> the dummy (0.5, 0.5) (utils/nn_utils.lua:378)"""
        if not self.normalized:
            if isinstance(self.data, nn_utils.DeviceTensor):
                raise L.GanrevError("normalize() of a device-resident result: load it with normalize=True (the fused launch ends in it)")
            nn_utils.normalize(self.data)
            self.normalized = True
        return 0.5, 0.5

    def free(self):
        if isinstance(self.data, nn_utils.DeviceTensor):
            self.data.free()


def _convert_group(ctx, arrays, rows, out, to, normalize, planes):
    """decoded files of ONE size -> their rows of out: one upload of the bytes, one gr_dataset_images_dev launch"""
    sh, sw, sc = arrays[0].shape
    n = len(arrays)
    per = planes * height * width
    stack = np.ascontiguousarray(np.stack(arrays))
    dbytes = ctx.upload(stack)
    consecutive = all(rows[k] + 1 == rows[k + 1] for k in range(n - 1))
    stage = None if consecutive else ctx.malloc(4 * n * per)
    try:
        ctx.dataset_images_dev(dbytes, n, sh, sw, sc, height, width, to, normalize, out.ptr + 4 * per * rows[0] if consecutive else stage)
        if stage is not None:                                             # a group scattered over the result: runs of rows move on the device
            k = 0
            while k < n:
                e = k + 1
                while e < n and rows[e] == rows[e - 1] + 1:
                    e += 1
                ctx.copy2d(out.ptr + 4 * per * rows[k], per, stage + 4 * per * k, per, e - k, per)
                k = e
        ctx.synchronize()                                                 # the byte buffer and the stage are freed below
    finally:
        ctx.free(dbytes)
        if stage is not None:
            ctx.free(stage)


def _load_decoding(ctx, files, grey_only, normalize, to, planes, out):
    """the drawn files, decoded now: groups of equal source size, one upload and one launch per group"""
    groups = {}                                                           # (sh, sw, sc) -> (arrays, rows) waiting for their launch
    for row, f in enumerate(files):
        a = decode(f)
        if grey_only and a.shape[2] != 1:
            raise L.GanrevError(f"{f}: {a.shape[2]} channels with nbChannels 1 (image.load's colour -> grey conversion is not restated)")
        arrays, rows = groups.setdefault(a.shape, ([], []))
        arrays.append(a); rows.append(row)
        if len(arrays) * a.nbytes >= CHUNK_BYTES:
            _convert_group(ctx, arrays, rows, out, to, normalize, planes)
            del groups[a.shape]
    for arrays, rows in groups.values():
        _convert_group(ctx, arrays, rows, out, to, normalize, planes)


def _load_cached(indices, files, grey_only, normalize, to, out):
    """the drawn images from the cache: the nbChannels 1 refusal from the host records, then ONE launch"""
    if grey_only:
        for i, f in zip(indices, files):
            sc = _cache.image(int(i))[2]
            if sc != 1:
                raise L.GanrevError(f"{f}: {sc} channels with nbChannels 1 (image.load's colour -> grey conversion is not restated)")
    if len(files):
        _cache.load_dev(indices, height, width, to, normalize, out.ptr)


def _load(indices, grey_only, normalize, device, ctx):
    if height < 1 or width < 1:
        raise L.GanrevError(f"dataset: height {height} and width {width} must be positive")
    if _cache is not None:
        if ctx is not None and ctx is not _cache.ctx:
            raise L.GanrevError("dataset: the cache lives on another context than the one this load names")
        ctx = _cache.ctx
    ctx = ctx or L.default_context()
    files = [paths[int(i)] for i in indices]
    to = L.COLOR_SPACES[colorSpace]
    planes = 1 if to == L.GR_CS_Y else 3
    out = nn_utils.DeviceTensor(ctx, (len(files), planes, height, width))
    try:
        if _cache is not None:
            _load_cached(indices, files, grey_only, normalize, to, out)
        else:
            _load_decoding(ctx, files, grey_only, normalize, to, planes, out)
    except BaseException:
        out.free()
        raise
    data = out
    if not device:
        data = out.numpy()
        out.free()
    return Images(data, np.asarray(indices, np.int64), files, bool(normalize))


def loadImages(startAt, count, normalize=False, device=True, ctx=None):
    """dataset.lua:99-131: `count` images from file number startAt (1-based) on, in path order"""
    if nbChannels not in (None, 1, 3):
        raise L.GanrevError(f"nbChannels {nbChannels}: 1 (grayscale) or 3 (color)")      # dataset.lua:59
    return _load(imageIndices(startAt, count), nbChannels == 1, normalize, device, ctx)


def loadRandomImages(count, seed=None, normalize=False, device=True, ctx=None):
    """dataset.lua:137-173: `count` randomly chosen images (always three channels in: image.load(fp, 3, "float"), :149)"""
    return _load(randomIndices(count, seed), False, normalize, device, ctx)
