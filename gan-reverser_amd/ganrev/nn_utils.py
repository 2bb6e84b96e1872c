"""Mirror of the hot-path helpers of utils/nn_utils.lua and of its colour-space conversions (:133-263, :324-379)."""
import contextlib

import numpy as np

from . import _lib as L
from . import synth


def forwardBatched(model, input, batchSize):
    """utils/nn_utils.lua:5-33 — chunked forward; the reference copies row by row in Lua (:25-28), here each chunk's
    result lands in the output with one strided copy."""
    N = len(input)
    output = None
    nBatches = -(-N // batchSize)
    for i in range(nBatches):
        s, e = i * batchSize, min((i + 1) * batchSize, N)
        forwarded = model.forward(input[s:e])
        if output is None:
            output = np.empty((N,) + forwarded.shape[1:], dtype=np.float32)
        output[s:e] = forwarded
    return output


class DeviceTensor:
    """A row-major fp32 tensor in GPU memory (what a torch.CudaTensor is to the reference's scripts): pointer + shape, nothing else.
    .numpy() copies it to the host; .free() releases it, and so does leaving a `with` block over it."""

    def __init__(self, ctx, shape, ptr=None):
        self.ctx, self.shape = ctx, tuple(int(s) for s in shape)
        self.size = int(np.prod(self.shape))
        self.owned = ptr is None
        self.ptr = ctx.malloc(4 * max(self.size, 1)) if ptr is None else ptr

    def rows(self, lo, hi=None):
        """view of rows [lo, hi)"""
        hi = self.shape[0] if hi is None else hi
        per = self.size // max(self.shape[0], 1)
        return DeviceTensor(self.ctx, (hi - lo,) + self.shape[1:], self.ptr + 4 * per * lo)

    def numpy(self):
        return self.ctx.download(self.ptr, self.shape)

    def free(self):
        if self.owned and self.ptr is not None:
            self.ctx.free(self.ptr)
        self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class DeviceScope(contextlib.ExitStack):
    """Owner of the device memory of one run or one step: a context manager that hands out DeviceTensors (tensor) and raw buffers (malloc,
    upload), adopts what was made elsewhere - a DeviceTensor, a pointer from ctx.malloc, anything with free() or close() - and on exit, however
    the block ends, releases what it still holds in reverse order.  release(t) does it early; each thing is released once."""

    def __init__(self, ctx):
        super().__init__()
        self.ctx, self.held = ctx, []

    def adopt(self, t):
        self.held.append(t)
        self.callback(self.release, t)
        return t

    def tensor(self, shape):
        return self.adopt(DeviceTensor(self.ctx, shape))

    def malloc(self, nbytes):
        return self.adopt(self.ctx.malloc(nbytes))

    def upload(self, arr):
        return self.adopt(self.ctx.upload(arr))

    def release(self, t):
        if t not in self.held:
            return
        self.held.remove(t)
        if isinstance(t, int):
            self.ctx.free(t)
        else:
            (t.free if hasattr(t, "free") else t.close)()


@contextlib.contextmanager
def deviceTable(ctx, table, rows=None):
    """A table [N x d] on the device, for the length of a block -> (pointer, N, d): a DeviceTensor as it lies; a host array uploaded to a temporary
    buffer, which is freed after the block once the context has synchronised (what the block enqueued may still read it).  rows=M: the first M rows."""
    if isinstance(table, DeviceTensor):
        N = table.shape[0]
        yield table.ptr, N if rows is None else rows, table.size // N
        return
    table = np.ascontiguousarray(table if rows is None else table[:rows], np.float32)
    ptr = ctx.upload(table)
    try:
        yield ptr, table.shape[0], table.size // table.shape[0]
    finally:
        try:
            ctx.synchronize()
        finally:
            ctx.free(ptr)


def forwardBatchedDev(model, input, batchSize, out=None):
    """utils/nn_utils.lua:5-33 with input and result resident on the GPU: `input` is a DeviceTensor [N x ...], the result a
    DeviceTensor [N x model output]; each chunk's last kernel writes its rows of the result itself (gr_net_forward_batched_dev) -
    the reference's per-row copy loop (:25-28) has no counterpart and nothing visits the host."""
    N = input.shape[0]
    net = model.device_net(input.shape[1:])
    shape = (N,) + L.Net._shape(net.out_dims)
    if out is None:
        out = DeviceTensor(input.ctx, shape)
    assert out.shape == shape, (out.shape, shape)
    net.forward_batched_dev(input.ptr, N, batchSize, out.ptr)
    return out


def createNoiseInputsDev(ctx, N, noiseDim, method="normal", seed=1):
    """utils/nn_utils.lua:39-51 drawn on the GPU (Philox4x32-10; the stream tests/test_gpu_abi_behaviour.py pins)."""
    t = DeviceTensor(ctx, (N, noiseDim))
    ctx.fill_noise(t.ptr, N * noiseDim, method, seed)           # ValueError for an unknown method (utils/nn_utils.lua:48)
    return t


def createNoiseInputs(N, noiseDim, method="normal", seed=1):
    """utils/nn_utils.lua:39-51 — N x noiseDim, normal(0,1) or uniform(-1,1)."""
    if method == "uniform":
        return synth.uniform((N, noiseDim), seed)
    if method == "normal":
        return synth.normal((N, noiseDim), seed)
    raise ValueError(f"Unknown noise method '{method}'")   # utils/nn_utils.lua:48


def createImagesFromNoise(model_g, noiseInputs, batchSize):
    """utils/nn_utils.lua:57-81 — G's images for every noise row, batchSize rows per forward (the reference reads MODEL_G and
    OPT.batchSize from globals; here they are arguments).  Always a tensor: outputAsList only changed the container."""
    return forwardBatched(model_g, noiseInputs, batchSize)


def createImages(model_g, N, noiseDim, batchSize, method="normal", seed=1):
    """utils/nn_utils.lua:83-91 — createImagesFromNoise(createNoiseInputs(N))."""
    return createImagesFromNoise(model_g, createNoiseInputs(N, noiseDim, method, seed), batchSize)


def predictionOrder(predictions, ascending, nbMaxOut):
    """The ordering step of sortImagesByPrediction (utils/nn_utils.lua:116-127): positions of the first min(nbMaxOut, N) predictions,
    ascending or descending.  Equal predictions keep ascending input order (a stable sort); the reference's table.sort is unstable,
    so its order among ties is unspecified."""
    p = np.asarray(predictions, dtype=np.float64).reshape(-1)
    order = np.argsort(p if ascending else -p, kind="stable")
    return order[:max(0, min(int(nbMaxOut), p.size))]


def sortImagesByPrediction(model_d, images, ascending, nbMaxOut, batchSize):
    """utils/nn_utils.lua:101-129 — D's prediction for every image (batchSize images per forward; D as it is, the caller puts it in
    evaluate mode as sample.lua:203 does), then the images ordered by it -> (images [m x C x H x W], predictions [m]),
    m = min(nbMaxOut, N).  Descending puts what D takes for real first.  Ties: see predictionOrder."""
    images = np.asarray(images, dtype=np.float32)
    predictions = forwardBatched(model_d, images, batchSize).reshape(len(images), -1)[:, 0]
    order = predictionOrder(predictions, ascending, nbMaxOut)
    return images[order], predictions[order]


# ---------------------------------------------------------------------------------------------------------------------
# Colour spaces (utils/nn_utils.lua:133-263).  Every conversion is one gr_colorspace_* call: a host array goes through
# gr_colorspace_host and comes back as a host array, a DeviceTensor goes through gr_colorspace_dev and comes back as a DeviceTensor.
def _cs(name, which):
    if name not in L.COLOR_SPACES:
        raise ValueError(f"Unknown color space <{which}>: '{name}'")        # utils/nn_utils.lua:165
    return L.COLOR_SPACES[name]


def _convert(images, from_, to):
    f, t = _cs(from_, "from"), _cs(to, "to")
    if f == L.GR_CS_RGB and t == L.GR_CS_RGB:
        return images                                                     # :148-149, :192-193: the tensor itself
    planes = 1 if t == L.GR_CS_Y else 3
    if isinstance(images, DeviceTensor):
        b, c, h, w = images.shape
        if c != (1 if f == L.GR_CS_Y else 3):
            raise ValueError(f"'{from_}' images have {1 if f == L.GR_CS_Y else 3} channel(s), not {c}")
        out = DeviceTensor(images.ctx, (b, planes, h, w))
        images.ctx.colorspace_dev(images.ptr, f, t, b, h, w, out.ptr)
        return out
    return L.default_context().colorspace(toImageTensor(images), f, t)


def toImageTensor(imageList):
    """utils/nn_utils.lua:269-307 without forceChannel: a list of [C x H x W] images becomes one [N x C x H x W] tensor"""
    return np.ascontiguousarray(imageList, dtype=np.float32)


def toBatch(image):
    """utils/nn_utils.lua:248-263: a batch of one"""
    return np.asarray(image)[None]


def toRgb(images, from_):
    """utils/nn_utils.lua:146-167"""
    return _convert(images, from_, "rgb")


def rgbToColorSpace(images, colorSpace):
    """utils/nn_utils.lua:191-217; an unknown target prints the reference's warning and returns None (:214)"""
    if colorSpace not in L.COLOR_SPACES:
        print("[WARNING] unknown color space in rgbToColorSpace: '" + str(colorSpace) + "'")
        return None
    return _convert(images, "rgb", colorSpace)


def switchColorSpace(images, from_, to):
    """utils/nn_utils.lua:133-137: toRgb then rgbToColorSpace, as ONE launch (the rgb intermediate is never written; bit-identical to
    the two calls).  Only rgb -> rgb passes through: y -> y, yuv -> yuv and hsl -> hsl go through rgb, as the reference does."""
    _cs(from_, "from")
    if to not in L.COLOR_SPACES:
        return rgbToColorSpace(images, to)
    return _convert(images, from_, to)


def switchColorSpaceSingle(image, from_, to):
    """utils/nn_utils.lua:139-144"""
    images = switchColorSpace(toBatch(image), from_, to)
    return None if images is None else images[0]


def rgb2y(im, threeChannels=False):
    """utils/nn_utils.lua:221-246: one [3 x H x W] image -> [1 x H x W] (or the plane three times) by 0.21 r + 0.72 g + 0.07 b"""
    im = np.asarray(im, dtype=np.float32)
    if im.shape[0] != 3:
        print("<error> expected 3 channels")                              # :224-227
        return im
    z = _convert(toBatch(im), "rgb", "y")[0]
    return np.repeat(z, 3, axis=0) if threeChannels else z


def normalize(data, mean_=None, std_=None):
    """utils/nn_utils.lua:324-379: in place from [0, 1] to [-1, 1] (x * 2 - 1, clamped); returns the reference's dummy (0.5, 0.5).
    NORMALIZE is false in every reference script, so this has no kernel: host numpy on a host array or a list of them."""
    for i in range(len(data)):
        d = data[i]
        d *= 2
        d += -1.0
        np.clip(d, -1.0, 1.0, out=d)
    return 0.5, 0.5
