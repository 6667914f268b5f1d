"""CPU: the reference of the float destinations (tests/floats.py) against values worked out by hand, and the checks
Context.decode_view_float makes before it calls the library — neither needs a device.

The hand-computed cases are the ones the contract of dwtx_decode_view_float (include/dwtx.h) names: the integers
themselves under the identity, round to nearest even in both half types, a float16 subnormal, overflow to infinity, and
scale and bias that belong to colours, not to memory positions."""
import struct

import numpy as np
import pytest

import floats


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def ref1(v, kind, scale=1.0, bias=0.0):
    return int(floats.reference(np.array([[v]]), kind, scale, bias)[0, 0])


def test_identity_gives_the_integers_in_all_three_types():
    v = np.arange(256).reshape(-1, 1)
    assert (floats.reference(v, "float32")[:, 0] == [f32_bits(float(i)) for i in range(256)]).all()
    assert (floats.reference(v, "float16")[:, 0] == np.arange(256).astype(np.float16).view(np.uint16)).all()
    # an integer up to 255 has at most 8 significant bits: a bfloat16 holds it, its bits are the float32's upper half
    assert (floats.reference(v, "bfloat16")[:, 0] == [f32_bits(float(i)) >> 16 for i in range(256)]).all()


def test_float16_rounds_to_nearest_even():
    # 11 significant bits: from 2048 on the spacing is 2, from 4096 on 4
    assert ref1(4095, "float16") == 0x6C00                      # 4096: the tie between 4094 and 4096 goes to the even mantissa
    assert ref1(2049, "float16") == 0x6800                      # 2048: the tie between 2048 and 2050 goes to the even mantissa
    assert ref1(2051, "float16") == 0x6802                      # 2052: the next tie goes up
    assert ref1(2050, "float16") == 0x6801                      # representable as it is
    assert np.array([0x6C00, 0x6800, 0x6802], dtype=np.uint16).view(np.float16).tolist() == [4096.0, 2048.0, 2052.0]


def test_bfloat16_rounds_to_nearest_even():
    # 8 significant bits: from 256 on the spacing is 2
    assert ref1(257, "bfloat16") == 0x4380                      # 256: the tie between 256 and 258, even mantissa
    assert ref1(259, "bfloat16") == 0x4382                      # 260: the tie between 258 and 260 goes up
    assert ref1(258, "bfloat16") == 0x4381
    assert ref1(4095, "bfloat16") == 0x4580                     # 4096 (spacing 16 there: 4095 is nearest to 4096)


def test_a_float16_subnormal_is_kept():
    assert ref1(3, "float16", scale=2.0 ** -24) == 0x0003       # 3 * 2^-24: three units of the last subnormal place
    assert ref1(1, "float16", scale=2.0 ** -20) == 0x0010
    assert ref1(1, "float16", scale=2.0 ** -25) == 0x0000       # the tie between 0 and 2^-24 goes to the even one


def test_float16_overflow_goes_to_infinity():
    assert ref1(65535, "float16") == 0x7C00
    assert ref1(65520, "float16") == 0x7C00                     # the tie between 65504 and 2^16
    assert ref1(65519, "float16") == 0x7BFF                     # 65504, the largest float16
    assert ref1(65535, "bfloat16") == 0x4780                    # 65536
    assert ref1(65535, "float32") == f32_bits(65535.0)


def test_two_roundings_not_one():
    """v * s + b with the product rounded to float32 first: 3 * (1/3 rounded) is 1 + 2^-25 before rounding and exactly 1
    after it, so 3 * s - 1 is 0 here, where a fused multiply-add gives 2^-25."""
    s = float(np.float32(1.0 / 3.0))
    assert ref1(3, "float32", scale=s, bias=-1.0) == 0
    fused = np.float32(np.float64(3.0) * np.float64(s) - 1.0)
    assert fused != 0


def test_scale_and_bias_belong_to_colours_under_bgr():
    v = np.array([[[1, 2, 3]]])
    rgb = floats.reference(v, "float32", scale=(10.0, 100.0, 1000.0), bias=(0.5, 0.25, 0.125), order="rgb")
    bgr = floats.reference(v, "float32", scale=(10.0, 100.0, 1000.0), bias=(0.5, 0.25, 0.125), order="bgr")
    assert rgb[0, 0].tolist() == [f32_bits(10.5), f32_bits(200.25), f32_bits(3000.125)]
    assert bgr[0, 0].tolist() == [f32_bits(3000.125), f32_bits(200.25), f32_bits(10.5)]   # memory: B, G, R — each with its own colour's pair
    gray = floats.reference(np.array([[[7]]]), "float16", scale=(2.0, 99.0, 99.0), bias=(1.0, 99.0, 99.0))
    assert gray[0, 0, 0] == np.float16(15.0).view(np.uint16)                               # gray uses [0]


def test_the_imagenet_set_follows_the_maxval():
    s255, b255 = floats.SETS["imagenet"](255)
    s4095, b4095 = floats.SETS["imagenet"](4095)
    assert b255 == b4095 and all(abs(a * 255 - b * 4095) < 1e-12 for a, b in zip(s255, s4095))
    assert abs(s255[0] * 255 * 0.229 - 1) < 1e-12 and abs(b255[2] + 0.406 / 0.225) < 1e-12
    assert len({*s255}) == 3 and len({*b255}) == 3   # three different pairs: a swap of colours shows


# ---- the checks of the Python layer: before any library call --------------------------------------------------------------

class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


@pytest.fixture
def bare():
    """A Context that was never opened: no device, no handle, and a library that must not be touched."""
    import torch

    import dwt_amd

    c = dwt_amd.Context.__new__(dwt_amd.Context)
    c.torch, c.lib, c.h, c.device = torch, NoLibrary(), None, torch.device("cpu")
    return c


def test_decode_view_float_refuses_bad_arguments_before_any_library_call(bare):
    import torch

    streams, lens = torch.zeros((2, 64), dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    good = torch.zeros((2, 8, 8, 3), dtype=torch.float32)
    for bad in (torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8, 3), dtype=torch.float64), torch.zeros((2, 8, 8, 3), dtype=torch.int16)):
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            bare.decode_view_float(streams, lens, bad)
    for kw in (dict(scale=(1.0, 2.0)), dict(bias=(0.0, 0.0, 0.0, 0.0)), dict(scale=[])):
        with pytest.raises(ValueError, match="one value or three"):
            bare.decode_view_float(streams, lens, good, **kw)
    for kw in (dict(scale=float("nan")), dict(bias=(0.0, float("inf"), 0.0)), dict(scale=(1.0, 1.0, -float("inf"))), dict(scale=1e39)):
        with pytest.raises(ValueError, match="not a finite float32"):
            bare.decode_view_float(streams, lens, good, **kw)
    with pytest.raises(ValueError, match="'rgb' or as 'bgr'"):
        bare.decode_view_float(streams, lens, good, order="rbg")


def test_decode_view_keeps_refusing_float_tensors(bare):
    import torch

    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="uint8 / uint16 / int16"):
            bare.decode_view(torch.zeros((2, 64), dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros((2, 8, 8, 3), dtype=dtype))


def test_float_format_holds_the_values_as_float32():
    import torch

    import dwt_amd

    f = dwt_amd.float_format(torch.bfloat16, 0.1, (1.0, 2.0, 3.0))
    assert f.type == 2 and list(f.scale) == [float(np.float32(0.1))] * 3 and list(f.bias) == [1.0, 2.0, 3.0]
    assert dwt_amd.float_format(torch.float32).type == 0 and dwt_amd.float_format("float16").type == 1
