"""CPU: float sources — tests/quant.py, the reference quantiser of dwtx_encode_view_float (include/dwtx.h), held to
hand-computed cases, to exact arithmetic and to torch's own line on the CPU; the pictures it makes for the GPU tests;
and the Python layer's checks, which run before any library call."""
from fractions import Fraction

import numpy as np
import pytest

import floats
import quant

KINDS = quant.KINDS


def q1(values, kind="float32", scale=1.0, bias=0.0, maxval=255, order="rgb"):
    """gray samples -> their integers"""
    bits = quant.to_bits(np.asarray(values, dtype=np.float64), kind).reshape(-1, 1)
    return quant.quantise(bits, kind, scale, bias, maxval, order)[:, 0].tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_hand_computed_cases(kind):
    inf, nan = float("inf"), float("nan")
    assert q1([0.5, 1.5, 2.5, 3.5, -0.4, -0.5, -0.0, 0.0], kind) == [0, 2, 2, 4, 0, 0, 0, 0]      # ties to even; below zero
    assert q1([255.5, 254.5, 256.0, 300.0, -7.0], kind) == [255, 254, 255, 255, 0]               # (255.5 -> 256 -> the clamp)
    assert q1([nan, inf, -inf], kind) == [0, 255, 0]
    assert q1([nan, inf, -inf, 5000.0], kind, maxval=4095) == [0, 4095, 0, 4095]
    assert q1([inf, 0.5, 1.0], kind, maxval=1) == [1, 0, 1]
    assert q1([-1.0, 0.0, 1.0, 2.0, -2.0], kind, *quant.UNIT) == [0, 128, 255, 255, 0]             # 127.5 -> 128: a tie, to even
    assert q1([1.25, 0.25, 0.75], kind, 2.0, 0.0) == [2, 0, 2]                                    # 2.5 -> 2, 0.5 -> 0, 1.5 -> 2


def test_the_half_types_widen_exactly():
    """Values float32 holds with room to spare but whose float16 / bfloat16 neighbours differ: the quantiser sees the
    sample's own value, not a rounded one."""
    # float16: 1 + 2^-10 is the value after 1; times 1024 that is 1025
    bits = np.array([[0x3C01]], dtype=np.uint16)
    assert quant.widen(bits, "float16")[0, 0] == np.float32(1 + 2.0 ** -10)
    assert quant.quantise(bits, "float16", 1024.0, 0.0, 4095)[0, 0] == 1025
    # float16 subnormal: 2^-24 is its smallest; scale 100 * 2^24 gives 100
    sub = np.array([[0x0001]], dtype=np.uint16)
    assert quant.widen(sub, "float16")[0, 0] == np.float32(2.0 ** -24)
    assert quant.quantise(sub, "float16", 100.0 * 2.0 ** 24, 0.0, 255)[0, 0] == 100
    # bfloat16: 1 + 2^-7 is the value after 1; times 128 that is 129
    bits = np.array([[0x3F81]], dtype=np.uint16)
    assert quant.widen(bits, "bfloat16")[0, 0] == np.float32(1 + 2.0 ** -7)
    assert quant.quantise(bits, "bfloat16", 128.0, 0.0, 255)[0, 0] == 129
    # and a bfloat16 beyond float16's range
    big = quant.to_bits(np.array([[1e6]]), "bfloat16")
    assert quant.quantise(big, "bfloat16", 1e-4, 0.0, 255)[0, 0] == int(np.rint(np.float32(quant.widen(big, "bfloat16")[0, 0]) * np.float32(1e-4)))


@pytest.mark.parametrize("kind", KINDS)
def test_scale_and_bias_follow_the_colours_not_the_memory_positions(kind):
    scale, bias = (1.0, 2.0, 4.0), (0.0, 10.0, 100.0)
    lies = quant.to_bits(np.array([[3.0, 5.0, 7.0]]), kind)          # one pixel, as it lies
    assert quant.quantise(lies, kind, scale, bias, 255).tolist() == [[3, 20, 128]]              # R = 3, G = 5, B = 7
    assert quant.quantise(lies, kind, scale, bias, 255, order="bgr").tolist() == [[7, 20, 112]]  # R = 7 * 1, G = 5 * 2 + 10, B = 3 * 4 + 100
    gray = quant.to_bits(np.array([[3.0]]), kind)
    assert quant.quantise(gray, kind, scale, bias, 255).tolist() == [[3]]                       # gray uses [0]


def fl32(x):
    """a rational -> the nearest float32 (ties to even), exactly, as a Fraction.  (Normal range only.)"""
    x = Fraction(x)
    if x == 0:
        return x
    e = 0
    a = abs(x)
    while a >= 2 ** 24:
        a /= 2
        e += 1
    while a < 2 ** 23:
        a *= 2
        e -= 1
    n, rest = divmod(a.numerator, a.denominator)
    twice = 2 * rest
    if twice > a.denominator or (twice == a.denominator and n % 2 == 1):
        n += 1
    r = Fraction(n) * Fraction(2) ** e
    return r if x > 0 else -r


def rint_exact(x):
    n, rest = divmod(x.numerator, x.denominator)   # floor
    twice = 2 * rest
    return n + 1 if twice > x.denominator or (twice == x.denominator and n % 2 == 1) else n


def test_two_roundings_not_one():
    """quant.WITNESS at scale = bias = 127.5, in exact arithmetic: the product rounded to float32 and then the sum rounded
    to float32 gives another integer than the exact product plus the bias rounded once (what a fused multiply-add
    computes).  The reference has two, and so has the contract."""
    x, s, b = Fraction(quant.WITNESS), Fraction(127.5), Fraction(127.5)
    assert fl32(x) == x and float(np.float32(quant.WITNESS)) == quant.WITNESS   # the witness is a float32
    two = rint_exact(fl32(fl32(x * s) + b))
    one = rint_exact(fl32(x * s + b))
    assert (two, one) == (20, 19)
    assert q1([quant.WITNESS], "float32", *quant.UNIT) == [20]
    # (the exact value lies just below the tie 19.5, the rounded product puts the sum exactly on it: 19.5 -> 20)
    assert x * s + b < Fraction(39, 2) and fl32(x * s) + b == Fraction(39, 2)


@pytest.mark.parametrize("name", list(quant.SETS))
@pytest.mark.parametrize("maxval", [255, 4095])
@pytest.mark.parametrize("kind", KINDS)
def test_the_reference_agrees_with_torchs_own_line_on_the_cpu(kind, maxval, name):
    """(x.float() * s + b).round().clamp(0, maxval) on the CPU, per colour, for every sample that is not a NaN (torch's
    clamp keeps those)."""
    import torch

    bits, v = quant.window(72, 68, 3, kind, maxval, name, 1)
    scale, bias = quant.SETS[name](maxval)
    x = torch.from_numpy(bits.copy().view(np.int32 if kind == "float32" else np.int16)).view(floats.torch_dtype(kind))
    s, b = torch.from_numpy(floats.three(scale)), torch.from_numpy(floats.three(bias))
    line = ((x.float() * s) + b).round().clamp(0, maxval)
    ok = ~torch.isnan(line)
    assert int((~ok).sum()) >= 1
    assert (line[ok].to(torch.int64).numpy() == v[ok.numpy()]).all()
    assert (v[~ok.numpy()] == 0).all()


SHAPES = [(256, 256), (132, 100), (72, 68), (64, 64), (8, 8), (37, 53), (130, 67)]   # tests/test_views_gpu.py's SHAPES


@pytest.mark.parametrize("name", list(quant.SETS))
@pytest.mark.parametrize("maxval", [255, 4095])
@pytest.mark.parametrize("kind", KINDS)
def test_every_picture_holds_the_planted_cases(kind, maxval, name):
    """A tie, a sample the clamp cuts on each side and a NaN in every generated picture; ties below an even and an odd
    integer wherever the type can reach them (tests/quant.py: with scale 1 in every type, at any scale in float32)."""
    scale, bias = quant.SETS[name](maxval)
    for W, H in SHAPES[1:]:
        for Cn in (1, 3):
            for order in ("rgb",) + (("bgr",) if Cn == 3 else ()):
                bits, v = quant.window(W, H, Cn, kind, maxval, name, 0, order)
                c = quant.census(bits, kind, scale, bias, maxval, order)
                assert c["nan"] >= 1 and c["low"] >= 1 and c["high"] >= 1, (W, H, Cn, order, c)
                if name != "imagenet_inv" or kind == "float32":
                    assert c["ties_even"] + c["ties_odd"] >= 1, (W, H, Cn, order, c)
                if name == "identity" or kind == "float32":
                    assert c["ties_even"] >= 1 and c["ties_odd"] >= 1, (W, H, Cn, order, c)
                assert v.min() == 0 and v.max() == maxval


def test_the_subnormal_float16_source_is_there():
    bits = quant.to_bits(np.array([[2.0 ** -24]]), "float16")
    assert bits[0, 0] == 1


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


def test_encode_view_float_refuses_bad_arguments_before_any_library_call(bare):
    import torch

    good = torch.zeros((2, 8, 8, 3), dtype=torch.float32)
    for bad in (torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8, 3), dtype=torch.float64), torch.zeros((2, 8, 8, 3), dtype=torch.int16)):
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            bare.encode_view_float(bad)
    for kw in (dict(scale=(1.0, 2.0)), dict(bias=(0.0, 0.0, 0.0, 0.0)), dict(scale=[])):
        with pytest.raises(ValueError, match="one value or three"):
            bare.encode_view_float(good, **kw)
    for kw in (dict(scale=float("nan")), dict(bias=(0.0, float("inf"), 0.0)), dict(scale=(1.0, 1.0, -float("inf"))), dict(scale=1e39)):
        with pytest.raises(ValueError, match="not a finite float32"):
            bare.encode_view_float(good, **kw)
    with pytest.raises(ValueError, match="'rgb' or as 'bgr'"):
        bare.encode_view_float(good, order="rbg")
    with pytest.raises(ValueError, match="1 or 3 channels"):
        bare.encode_view_float(torch.zeros((2, 8, 8, 2), dtype=torch.float16))


def test_encode_view_keeps_refusing_float_tensors(bare):
    import torch

    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="uint8 / uint16 / int16"):
            bare.encode_view(torch.zeros((2, 8, 8, 3), dtype=dtype))


def test_the_symbol_is_declared_exported_and_typed():
    """(tests/test_abi.py holds header, exports and table together; this names the new entry)"""
    from dwt_amd import _lib

    assert "dwtx_encode_view_float" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "dwtx_encode_view_float")
    assert len(_lib.SYMBOLS["dwtx_encode_view_float"][1]) == 12
