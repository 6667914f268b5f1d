"""CPU: signed 16-bit samples on the oracle (tests/signed.py) — the clamps and the quantiser by hand, exact round trips, the
plane bound for ranges of 4095 wherever they lie, the condition the clamp fixtures of tests/test_signed_gpu.py must meet,
and the four entry points declared, typed and exported."""
import re

import numpy as np
import pytest

import deep
import orc
import signed
import test_deep_cpu as D


# ---- by hand ---------------------------------------------------------------------------------------------------------------------

def test_gray_clamps_by_hand():
    img = np.array([[[-2000], [0], [5000]]])
    assert signed.clamp_pixels(img, 1, -1024, 3071).tolist() == [[[-1024], [0], [3071]]]
    assert signed.clamp_pixels(img, 1, -32768, 32767).tolist() == [[[-2000], [0], [5000]]]
    assert signed.clamp_pixels(img, 1, 0, 4095).tolist() == deep.to_pixels(img, 1, 4095).tolist() == [[[0], [0], [4095]]]
    assert signed.clamp_pixels(img, 1, 5, 100).tolist() == [[[5], [5], [100]]]


def test_rgb_clamps_by_hand():
    """[-2048, 2047], R = 4095.  Pixel 0: Co = 9000 -> 4095, Cg = -9000 -> -4095; T = 100 - (-4095 / 2) = 100 + 2047 = 2147,
    G = -4095 + 2147 = -1948, B = 2147 - 4095 / 2 = 100, R = 100 + 4095 = 4195 -> 2047.  Pixels 1 and 2: Y beyond either end, no
    chroma: all three channels at the bound.  Pixel 3: nothing to clamp before the colour transform (Co = -4095 is inside
    [-R, R] though outside [-maxval, maxval]): T = 0, G = 0, B = 0 - (-4095 / 2) = 2047, R = 2047 - 4095 = -2048."""
    img = np.array([[[100, 9000, -9000], [5000, 0, 0], [-5000, 0, 0], [0, -4095, 0]]])
    want = [[[2047, -1948, 100], [2047, 2047, 2047], [-2048, -2048, -2048], [-2048, 0, 2047]]]
    assert signed.clamp_pixels(img, 3, -2048, 2047).tolist() == want
    # with minval 0 the clamps are today's
    for M in (255, 4095):
        rnd = np.random.default_rng(M).integers(-3 * M, 3 * M, (5, 7, 3))
        assert (signed.clamp_pixels(rnd, 3, 0, M) == deep.to_pixels(rnd, 3, M)).all()


def test_quantiser_by_hand():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, np.nan, np.inf, -np.inf, -0.0, 1e9, -1e9, 3071.5, -1024.5], dtype=np.float32)[:, None]
    assert signed.quantise(x, 1.0, 0.0, -1024, 3071)[:, 0].tolist() == [0, 2, 2, 0, -2, -2, 0, 3071, -1024, 0, 3071, -1024, 3071, -1024]
    # NaN -> 0, clamped INTO the range: a range that does not hold 0 sends it to the nearer bound
    assert signed.quantise(x[6:10], 1.0, 0.0, 5, 100)[:, 0].tolist() == [5, 100, 5, 5]
    assert signed.quantise(x[6:10], 1.0, 0.0, -100, -5)[:, 0].tolist() == [-5, -5, -100, -5]
    # two roundings: 0.1f * 25 = 2.5000000373 rounds to 2.5f, + 0 -> tie -> 2; per-colour scale and bias
    y = np.array([[0.1, 0.1, -0.1]], dtype=np.float32)
    assert signed.quantise(y, [25.0, 35.0, 25.0], [0.0, 0.0, -1.0], -2048, 2047).tolist() == [[2, 4, -4]]


# ---- round trips -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", signed.RANGES + [signed.FULL], ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", signed.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_pictures_round_trip(wh, C, rng):
    (W, H), (lo, hi) = wh, rng
    pic, data, st = signed.stream("smooth_noise", W, H, C, lo, hi, 1)
    assert pic.dtype == np.int16 and pic.min() < 0 < pic.max() and pic.min() >= lo and pic.max() <= hi
    assert max(list(st.planes)[:C]) <= 16
    g = orc.geometry(W, H)   # channel 0's root image holds negative values: no unsigned picture's does
    assert orc.forward(deep.rgb2ycocg(pic) if C == 3 else pic.astype(np.int32))[:g.heights[0], :g.widths[0], 0].min() < 0
    back = signed.signed_decode(data, W, H, C, lo, hi)
    assert back.dtype == np.int16 and back.shape == pic.shape and (back == pic).all()
    # the stream is the shifted unsigned picture's but for the root image
    shifted = deep.deep_encode((pic.astype(np.int64) - lo).astype(np.uint16))
    print(W, H, C, rng, list(st.planes)[:C], len(data), len(shifted[0]))
    assert list(shifted[1].planes)[1:C] == list(st.planes)[1:C]


def test_the_uint16_reading_of_a_zero_crossing_picture():
    """What the keyword-less calls make of an int16 tensor that crosses zero: 17 planes, refused; as signed integers 7."""
    z = signed.zero_crossing(132, 72, 1)
    assert z.min() < 0 < z.max()
    assert list(deep.deep_encode(z)[1].planes)[:1] == [7]
    assert list(deep.deep_encode(z.view(np.uint16))[1].planes)[:1] == [17]


# ---- the plane bound ---------------------------------------------------------------------------------------------------------------

_gain = {}


def _detail_top(pic):
    """The largest |detail coefficient| of a picture through the integer transform (the root image is no coefficient)."""
    H, W, C = pic.shape
    g = orc.geometry(W, H)
    pyr = orc.forward(deep.rgb2ycocg(pic) if C == 3 else pic.astype(np.int32))
    pyr[:g.heights[0], :g.widths[0]] = 0
    return int(np.abs(pyr).max())


@pytest.mark.parametrize("wh", D.GEOMETRIES, ids=lambda wh: "%dx%d" % wh)
def test_a_range_of_4095_never_needs_more_than_16_planes(wh):
    """deep.Gain's worst-case pictures for R = 4095 (gray also R = 8191), shifted by minval: a shift moves the root image and,
    through the roundings alone, a detail coefficient by a count or two — the bound of DESIGN.md section 4.8 is the range's,
    wherever the range lies."""
    g = _gain.setdefault(wh, deep.Gain(*wh))
    for minval in (-4095, -2048, -1):
        for pic, R in ((g.worst_gray(4095), 4095), (g.worst_rgb(4095), 4095), (g.worst_gray(8191), 8191)):
            top = _detail_top(pic.astype(np.int64) + minval)
            print(wh, minval, R, pic.shape[2], top)
            assert top < 1 << 16, (minval, R, pic.shape[2])


# ---- the clamp fixtures ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", signed.RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", signed.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_clamp_fixtures_meet_their_condition(wh, C, rng):
    (W, H), (lo, hi) = wh, rng
    for cut in signed.CUTS:
        r = deep.decoded(signed.cut_fixture(W, H, C, lo, hi, cut), W, H, C)
        assert r is not None
        print(wh, C, rng, cut, "level", r[0], signed.clamp_shares(r[3], C, lo, hi))
        assert r[0] == orc.geometry(W, H).levels - 1
        assert signed.clamps_are_at_work(r[3], W, H, C, lo, hi)
        # and the clamps change the result
        assert (signed.signed_decode(signed.cut_fixture(W, H, C, lo, hi, cut), W, H, C, lo, hi) !=
                signed.clamp_pixels(r[3], C, -32768, 32767)).mean() > 0.2


def test_checker_and_noise_are_no_clamp_fixtures():
    W, H, lo, hi = 132, 72, -1024, 3071
    for pic in (deep.checker(W, H, 3, hi - lo).astype(np.int64) + lo, signed.noise(W, H, 3, lo, hi, 3)):
        data = deep.deep_encode(pic)[0]
        for cut in signed.CUTS:
            r = deep.decoded(data[:int(len(data) * cut)], W, H, 3)
            assert not signed.clamps_are_at_work(r[3], W, H, 3, lo, hi)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

SIGNED_SYMBOLS = ["dwtx_encode_view_signed", "dwtx_decode_view_signed", "dwtx_encode_images_s16", "dwtx_decode_images_s16"]


def test_signed_entry_points_are_declared_typed_and_exported():
    from dwt_amd import _lib
    import dwt_amd
    import test_abi

    lib = _lib.load()
    declared = test_abi.declared_symbols()
    for name in SIGNED_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/dwtx.h"
        assert name in _lib.SYMBOLS, f"{name} is not typed in dwt_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libdwtx.so"
    # the signed calls are the flip calls plus one int
    for d in ("encode", "decode"):
        flip, sgn = _lib.SYMBOLS["dwtx_%s_view_flip" % d][1], _lib.SYMBOLS["dwtx_%s_view_signed" % d][1]
        assert len(sgn) == len(flip) + 1
    text = open(orc.ROOT + "/include/dwtx.h").read()
    for d in ("encode", "decode"):
        args = re.search(r"int dwtx_%s_view_signed\((.*?)\);" % d, text, flags=re.S).group(1)
        assert "int minval" in args
    for m in ("encode16s", "decode16s"):
        assert callable(getattr(dwt_amd.Context, m))
    import inspect
    for m in ("encode_view", "decode_view", "decode_view_crop", "encode_view_list", "decode_view_list"):
        assert "signed" in inspect.signature(getattr(dwt_amd.Context, m)).parameters, m
    for m in ("encode_view_float", "decode_view_float", "decode_view", "decode_view_crop", "decode_view_list"):
        assert "minval" in inspect.signature(getattr(dwt_amd.Context, m)).parameters, m
