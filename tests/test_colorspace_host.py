"""not-gpu: the colour-space oracle (tests/colorspace_oracle.py) against Python's colorsys, known answers and its own float64 form, and the
parts of ganrev.nn_utils' colour-space surface that need no GPU (normalize, argument checks, the reference's warning).

The bars: the float64 HSL pair is a handful of float64 roundings on values of size at most 6 (below 1e-14), held to colorsys at 1e-12;
the fp32 twin against float64 is a sanity bar (a few fp32 ulps of values of size <= 6, amplified by 1 / d for the hue); the yuv round trip
is bounded by the five published digits of the constants times the largest coefficient (2.04), 1e-4.
"""
import colorsys

import numpy as np
import pytest

import colorspace_oracle as co


def _pixels(n, seed):
    return np.random.default_rng(seed).random((n, 3, 1, 1))


def _px(r, g, b):
    return np.array([r, g, b], np.float64).reshape(1, 3, 1, 1)


def test_float64_hsl_pair_matches_colorsys():
    x = _pixels(65536, 1)
    hsl = co.from_rgb(x, "hsl", np.float64)
    ref = np.array([colorsys.rgb_to_hls(*p) for p in x.reshape(-1, 3)])          # colorsys orders the triple h, l, s
    dh = np.abs(hsl[:, 0, 0, 0] - ref[:, 0]); dh = np.minimum(dh, 1 - dh)         # hue is compared modulo 1
    assert dh.max() < 1e-12, dh.max()
    assert np.abs(hsl[:, 2, 0, 0] - ref[:, 1]).max() < 1e-12
    assert np.abs(hsl[:, 1, 0, 0] - ref[:, 2]).max() < 1e-12
    hsl_in = _pixels(65536, 2)
    rgb = co.to_rgb(hsl_in, "hsl", np.float64)
    ref = np.array([colorsys.hls_to_rgb(h, l, s) for h, s, l in hsl_in.reshape(-1, 3)])
    assert np.abs(rgb.reshape(-1, 3) - ref).max() < 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_known_answers(dtype):
    tol = 1e-15 if dtype == np.float64 else 1e-6
    hsl = lambda r, g, b: co.from_rgb(_px(r, g, b), "hsl", dtype).reshape(3).astype(np.float64)
    assert hsl(1, 1, 1).tolist() == [0, 0, 1]                                     # white
    assert hsl(0, 0, 0).tolist() == [0, 0, 0]                                     # black
    assert hsl(0.25, 0.25, 0.25).tolist() == [0, 0, 0.25]                         # a gray: h = s = 0, l = the value
    np.testing.assert_allclose(hsl(1, 0, 0), [0, 1, 0.5], atol=tol)               # the three primaries
    np.testing.assert_allclose(hsl(0, 1, 0), [1 / 3, 1, 0.5], atol=tol)
    np.testing.assert_allclose(hsl(0, 0, 1), [2 / 3, 1, 0.5], atol=tol)
    np.testing.assert_allclose(hsl(1, 0, 0.5), [(-0.5 + 6) / 6, 1, 0.5], atol=tol)      # mx == r and g < b: the +6 branch
    np.testing.assert_allclose(hsl(1, 1, 0), [1 / 6, 1, 0.5], atol=tol)           # tie mx == r == g: the r branch, (g - b) / d = 1
    np.testing.assert_allclose(hsl(0.5, 0.5, 0.25), [1 / 6, 1 / 3, 0.375], atol=tol)
    for rgb in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0.2, 0.4, 0.6]):
        back = co.to_rgb(co.from_rgb(_px(*rgb), "hsl", dtype), "hsl", dtype).reshape(3)
        np.testing.assert_allclose(back, rgb, atol=10 * tol)
    yuv = co.from_rgb(_px(1, 1, 1), "yuv", np.float64).reshape(3)
    np.testing.assert_allclose(yuv, [1, 1e-5, 0], atol=1e-12)                     # the published u row sums to 1e-5, not 0
    assert co.to_rgb(np.full((2, 1, 3, 3), 0.3), "y", dtype).shape == (2, 3, 3, 3)


def test_rgb2y_of_white():
    assert co.from_rgb(_px(1, 1, 1), "y", np.float64).reshape(()) == 1.0
    f = np.float32
    twin = co.from_rgb(_px(1, 1, 1), "y", np.float32).reshape(())
    assert twin.dtype == np.float32
    assert twin == (f(0.21) + f(0.72)) + f(0.07)                                  # whatever that rounds to in fp32, not 1
    yy = co.switch(np.full((1, 1, 1, 1), 0.5, np.float32), "y", "y").reshape(())
    assert yy == (f(0.21) * f(0.5) + f(0.72) * f(0.5)) + f(0.07) * f(0.5)         # y -> y goes through rgb


def test_fp32_twin_against_float64():
    x32 = _pixels(100000, 3).astype(np.float32)
    x64 = x32.astype(np.float64)
    for to in ("y", "yuv"):
        d = np.abs(co.from_rgb(x32, to) - co.from_rgb(x64, to, np.float64)).max()
        assert d < 1e-6, (to, d)
    yuv32 = co.from_rgb(x32, "yuv")
    assert np.abs(co.to_rgb(yuv32, "yuv") - co.to_rgb(yuv32.astype(np.float64), "yuv", np.float64)).max() < 1e-6
    h32, h64 = co.from_rgb(x32, "hsl"), co.from_rgb(x64, "hsl", np.float64)
    spread = (x64.max(axis=1) - x64.min(axis=1)).reshape(-1)
    excluded = spread < 1e-3                                                      # hue = (difference of two values) / d: ill-conditioned there
    assert excluded.mean() < 1e-3, excluded.mean()
    dh = np.abs(h32[:, 0] - h64[:, 0]).reshape(-1); dh = np.minimum(dh, 1 - dh)
    # numerator and d each carry one fp32 rounding of values <= 1 (6e-8 each), divided by d >= 1e-3 and by 6: 2e-5 plus the quotient's own ulps
    assert dh[~excluded].max() < 1e-4, dh[~excluded].max()
    assert np.abs(h32[:, 2] - h64[:, 2]).max() < 1e-6                             # l
    # s divides d by mx + mn or 2 - mx - mn, either of which may be tiny for near-black / near-white pixels: relative to 1 / that divisor
    div = np.where(h64[:, 2] > 0.5, 2 - x64.max(axis=1) - x64.min(axis=1), x64.max(axis=1) + x64.min(axis=1))
    assert (np.abs(h32[:, 1] - h64[:, 1]) * div).max() < 1e-6
    hsl32 = _pixels(100000, 4).astype(np.float32)
    assert np.abs(co.to_rgb(hsl32, "hsl") - co.to_rgb(hsl32.astype(np.float64), "hsl", np.float64)).max() < 5e-6


def test_yuv_round_trip_is_not_an_identity_but_close():
    x = _pixels(65536, 5).astype(np.float32)
    d = np.abs(co.switch(x, "rgb", "yuv") - 0).max()
    assert d <= 1.0001
    back = co.to_rgb(co.from_rgb(x, "yuv"), "yuv")
    err = np.abs(back - x).max()
    assert 0 < err < 1e-4, err          # measured 2.1e-5: the published constants are truncated to five digits


def test_fused_switch_is_the_two_steps():
    for f in co.SPACES:
        x = co.make_images((2, 4, 4), f, 7)
        for t in co.SPACES:
            a = co.switch(x, f, t)
            b = co.from_rgb(co.to_rgb(x, f), t)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert a.shape == (2, co.PLANES[t], 4, 4)
            assert np.isfinite(a).all() or t == "hsl"


def test_normalize_is_in_place_and_returns_the_dummy_pair():
    from ganrev import nn_utils
    data = np.array([[[[0.0, 0.25], [0.5, 1.0]]], [[[-0.5, 1.5], [0.75, 0.1]]]], np.float32)
    keep = data
    assert nn_utils.normalize(data) == (0.5, 0.5)
    assert keep is data
    np.testing.assert_array_equal(data[0, 0], [[-1.0, -0.5], [0.0, 1.0]])
    np.testing.assert_array_equal(data[1, 0], np.array([[-1.0, 1.0], [0.5, np.float32(0.1) * 2 - 1]], np.float32))
    lst = [np.full((1, 2, 2), 0.75, np.float32)]
    nn_utils.normalize(lst, 0.1, 0.2)                                             # mean_ / std_ are ignored (utils/nn_utils.lua:321-322)
    assert (lst[0] == 0.5).all()


def test_argument_and_warning_behaviour(capsys):
    from ganrev import nn_utils
    x = np.zeros((1, 3, 2, 2), np.float32)
    with pytest.raises(ValueError, match="Unknown color space <from>: 'lab'"):
        nn_utils.toRgb(x, "lab")
    with pytest.raises(ValueError, match="Unknown color space <from>"):
        nn_utils.switchColorSpace(x, "gray", "rgb")
    assert nn_utils.rgbToColorSpace(x, "lab") is None
    assert "[WARNING] unknown color space in rgbToColorSpace: 'lab'" in capsys.readouterr().out
    assert nn_utils.switchColorSpace(x, "rgb", "lab") is None                     # toRgb passes, rgbToColorSpace warns
    assert "[WARNING]" in capsys.readouterr().out
    assert nn_utils.toRgb(x, "rgb") is x and nn_utils.rgbToColorSpace(x, "rgb") is x      # the tensor itself, as :148-149 / :192-193
    assert nn_utils.switchColorSpace(x, "rgb", "rgb") is x
    assert nn_utils.toBatch(x[0]).shape == (1, 3, 2, 2)
    one = np.zeros((1, 2, 2), np.float32)
    assert nn_utils.rgb2y(one) is not None and nn_utils.rgb2y(one).shape == (1, 2, 2)     # "<error> expected 3 channels": the image back
    assert "expected 3 channels" in capsys.readouterr().out


def test_constants_and_symbols_are_bound():
    import ganrev._lib as L
    assert (L.GR_CS_RGB, L.GR_CS_Y, L.GR_CS_YUV, L.GR_CS_HSL) == (0, 1, 2, 3)
    assert [L.COLOR_SPACES[s] for s in co.SPACES] == [0, 1, 2, 3]
    assert {"gr_colorspace_dev", "gr_colorspace_host"} <= set(L.EXPORTED_SYMBOLS)
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "ganrev.h")).read()
    assert "utils/nn_utils.lua:133-246" in hdr
