"""gpu: gr_colorspace_dev / gr_colorspace_host (NN_UTILS.switchColorSpace, utils/nn_utils.lua:133-246) against the fp32 twin of
tests/colorspace_oracle.py, bit for bit: all 16 (from, to) pairs, the scalar and the 16-byte kernel forms, a misaligned allocation, the
fused switch against two single-step calls, the pass-through, the error paths, the nn_utils surface and the launch counts.

"Bit for bit" means np.array_equal on the uint32 views: no tolerance.  It holds because every operation of the kernel is one IEEE fp32
operation in the order the twin states (elem.hip is compiled with -ffp-contract=off and `/` is the correctly rounded division)."""
import ctypes as C

import numpy as np
import pytest

import colorspace_oracle as co

pytestmark = pytest.mark.gpu

PAIRS = [(f, t) for f in co.SPACES for t in co.SPACES]
# (batch, h, w): 7 * 9 = 63 pixels per plane -> the scalar form; 32 * 32 and 64 * 64 -> the 16-byte form
SHAPES = [(5, 7, 9), (130, 32, 32), (3, 64, 64)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bit_identical(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = bits(got) == bits(want)
    if not same.all():
        i = np.argwhere(~same)[0]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} values differ; first at {tuple(i)}: "
                             f"device {got[tuple(i)]!r} ({bits(got)[tuple(i)]:#x}) != twin {want[tuple(i)]!r} ({bits(want)[tuple(i)]:#x})")


def cs(name):
    import ganrev._lib as L
    return L.COLOR_SPACES[name]


def dev_switch(ctx, x, f, t, offset_floats=0):
    """gr_colorspace_dev on an upload of x -> host array; offset_floats shifts both tensors inside their allocations"""
    n, _, h, w = x.shape
    nout = n * co.PLANES[t] * h * w
    din = ctx.malloc(4 * (x.size + offset_floats))
    dout = ctx.malloc(4 * (nout + offset_floats))
    try:
        ctx.upload(x, din + 4 * offset_floats)
        ctx.colorspace_dev(din + 4 * offset_floats, cs(f), cs(t), n, h, w, dout + 4 * offset_floats)
        return ctx.download(dout + 4 * offset_floats, (n, co.PLANES[t], h, w))
    finally:
        ctx.free(din); ctx.free(dout)


def kernels_of(ctx, fn):
    ctx.set_timing(2)
    try:
        out = fn()
        kt = [k for k in ctx.kernel_times() if k["kernel"] != "range_guard_fallback"]
    finally:
        ctx.set_timing(0)
    return out, kt


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("f,t", PAIRS, ids=lambda v: v)
def test_every_pair_is_bit_identical_to_the_twin(ctx, f, t, shape):
    x = co.make_images(shape, f, 11 + 4 * cs(f) + cs(t))
    want = co.switch(x, f, t)
    assert_bit_identical(dev_switch(ctx, x, f, t), want, f"gr_colorspace_dev {f}->{t} {shape}")
    assert_bit_identical(ctx.colorspace(x, cs(f), cs(t)), want, f"gr_colorspace_host {f}->{t} {shape}")


@pytest.mark.parametrize("f,t", PAIRS, ids=lambda v: v)
def test_a_tensor_4_bytes_into_its_allocation_takes_the_scalar_form(ctx, f, t):
    """h * w % 4 == 0 but the pointers are only 4-byte aligned: the 16-byte form would fault or read the wrong pixels"""
    x = co.make_images((3, 16, 16), f, 90 + cs(f))
    (got, kt) = kernels_of(ctx, lambda: dev_switch(ctx, x, f, t, offset_floats=1))
    assert_bit_identical(got, co.switch(x, f, t), f"{f}->{t} at +4 bytes")
    if (f, t) != ("rgb", "rgb"):
        assert [(k["kernel"], k["launches"]) for k in kt] == [("colorspace_kernel", 1)], kt


@pytest.mark.parametrize("f", ["y", "yuv", "hsl"])
@pytest.mark.parametrize("t", ["y", "yuv", "hsl"])
def test_fused_switch_equals_two_single_steps(ctx, f, t):
    for shape in ((4, 32, 32), (2, 5, 7)):
        x = co.make_images(shape, f, 40 + cs(f))
        rgb = dev_switch(ctx, x, f, "rgb")
        assert_bit_identical(dev_switch(ctx, x, f, t), dev_switch(ctx, rgb, "rgb", t), f"{f}->{t} fused against {f}->rgb->{t} {shape}")


def test_rgb_to_rgb_copies_and_launches_nothing(ctx):
    x = co.make_images((3, 8, 8), "rgb", 5)
    got, kt = kernels_of(ctx, lambda: dev_switch(ctx, x, "rgb", "rgb"))
    assert_bit_identical(got, x, "rgb->rgb copy")
    assert kt == [], kt
    assert_bit_identical(ctx.colorspace(x, cs("rgb"), cs("rgb")), x, "rgb->rgb host copy")


def test_one_launch_per_call(ctx):
    for shape, name in (((4, 32, 32), "colorspace_kernel_v4"), ((4, 5, 7), "colorspace_kernel")):
        for f, t in PAIRS:
            if (f, t) == ("rgb", "rgb"):
                continue
            x = co.make_images(shape, f, 3)
            _, kt = kernels_of(ctx, lambda: dev_switch(ctx, x, f, t))
            assert [(k["kernel"], k["launches"]) for k in kt] == [(name, 1)], (f, t, shape, kt)
            n, _, h, w = x.shape
            assert kt[0]["bytes"] == 4 * (co.PLANES[f] + co.PLANES[t]) * n * h * w


def test_in_place_with_equal_plane_counts(ctx):
    for f, t in (("rgb", "hsl"), ("yuv", "rgb"), ("y", "y"), ("hsl", "hsl")):
        x = co.make_images((6, 16, 16), f, 8)
        d = ctx.upload(x)
        try:
            ctx.colorspace_dev(d, cs(f), cs(t), 6, 16, 16, d)
            assert_bit_identical(ctx.download(d, x.shape), co.switch(x, f, t), f"in place {f}->{t}")
        finally:
            ctx.free(d)


def test_bad_arguments_return_an_error_and_leave_out_untouched(ctx):
    import ganrev._lib as L
    x = co.make_images((2, 4, 4), "rgb", 1)
    sentinel = np.full(2 * 3 * 4 * 4, 7.25, np.float32)
    din, dout = ctx.upload(x), ctx.upload(sentinel)
    hout = sentinel.copy()
    p = lambda a: C.c_void_p(a) if isinstance(a, int) else (None if a is None else C.c_void_p(a.ctypes.data))
    try:
        cases = [  # (in, from, to, batch, h, w, out), message
            ((din, 4, 0, 2, 4, 4, dout), "<from>"), ((din, -1, 0, 2, 4, 4, dout), "<from>"), ((din, 0, 4, 2, 4, 4, dout), "<to>"),
            ((din, 0, 2, 2, 0, 4, dout), "positive"), ((din, 0, 2, 2, 4, -3, dout), "positive"), ((din, 0, 2, 0, 4, 4, dout), "positive"),
            ((None, 0, 2, 2, 4, 4, dout), "null"), ((din, 0, 2, 2, 4, 4, None), "null"),
            ((dout, 0, 1, 2, 4, 4, dout), "in place"), ((dout, 1, 3, 2, 4, 4, dout), "in place"),
        ]
        for (a_in, f, t, b, h, w, a_out), msg in cases:
            rc = ctx.lib.gr_colorspace_dev(ctx.h, p(a_in), f, t, b, h, w, p(a_out))
            assert rc == -1, (rc, msg)
            assert msg in ctx.lib.gr_last_error(ctx.h).decode(), (msg, ctx.lib.gr_last_error(ctx.h))
            hin = None if a_in is None else (hout if a_in == dout else x)
            rc = ctx.lib.gr_colorspace_host(ctx.h, p(hin), f, t, b, h, w, None if a_out is None else p(hout))
            assert rc == -1, (rc, msg)
            assert msg in ctx.lib.gr_last_error(ctx.h).decode()
        assert np.array_equal(ctx.download(dout, sentinel.shape), sentinel)
        assert np.array_equal(hout, sentinel)
        with pytest.raises(L.GanrevError, match="<to>"):
            ctx.colorspace_dev(din, 0, 9, 2, 4, 4, dout)
        with pytest.raises(L.GanrevError):
            ctx.colorspace(np.zeros((2, 1, 4, 4), np.float32), cs("rgb"), cs("y"))      # one plane is not an rgb image
    finally:
        ctx.free(din); ctx.free(dout)


def test_nn_utils_on_a_device_tensor_and_on_the_host_array_agree(ctx):
    from ganrev import nn_utils
    for f, t in PAIRS:
        x = co.make_images((4, 8, 12), f, 21)
        dt = nn_utils.DeviceTensor(ctx, x.shape)
        try:
            ctx.upload(x, dt.ptr)
            on_dev = nn_utils.switchColorSpace(dt, f, t)
            on_host = nn_utils.switchColorSpace(x, f, t)
            assert isinstance(on_dev, nn_utils.DeviceTensor) and isinstance(on_host, np.ndarray)
            assert on_dev.shape == on_host.shape == (4, co.PLANES[t], 8, 12)
            assert_bit_identical(on_dev.numpy(), on_host, f"nn_utils.switchColorSpace {f}->{t}")
            assert_bit_identical(on_host, co.switch(x, f, t), f"nn_utils.switchColorSpace {f}->{t} against the twin")
            if on_dev is not dt:
                on_dev.free()
        finally:
            dt.free()


def test_nn_utils_names(ctx):
    from ganrev import nn_utils
    y = co.make_images((2, 6, 6), "y", 2)
    assert nn_utils.toRgb(y, "y").shape[1] == 3
    rgb = co.make_images((2, 6, 6), "rgb", 2)
    for t in ("y", "yuv", "hsl"):
        assert_bit_identical(nn_utils.rgbToColorSpace(rgb, t), co.from_rgb(rgb, t), f"rgbToColorSpace {t}")
        assert_bit_identical(nn_utils.toRgb(co.make_images((2, 6, 6), t, 3), t), co.to_rgb(co.make_images((2, 6, 6), t, 3), t), f"toRgb {t}")
    assert_bit_identical(nn_utils.switchColorSpaceSingle(rgb[0], "rgb", "hsl"), co.switch(rgb[:1], "rgb", "hsl")[0], "switchColorSpaceSingle")
    z = nn_utils.rgb2y(rgb[0])
    assert z.shape == (1, 6, 6)
    assert_bit_identical(z, co.from_rgb(rgb[:1], "y")[0], "rgb2y")
    z3 = nn_utils.rgb2y(rgb[0], True)
    assert z3.shape == (3, 6, 6) and np.array_equal(z3[0], z[0]) and np.array_equal(z3[2], z[0])
    white = nn_utils.rgb2y(np.ones((3, 1, 1), np.float32))
    assert white.reshape(()) == (np.float32(0.21) + np.float32(0.72)) + np.float32(0.07)
    assert_bit_identical(nn_utils.toRgb([rgb[0], rgb[1]], "yuv"), co.to_rgb(rgb, "yuv"), "toRgb on a list of images")
