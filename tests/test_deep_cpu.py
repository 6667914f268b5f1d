"""CPU: the composed oracle for deep pixels (tests/deep.py) is pinned on the whole-file oracle and on the reference
binary's bytes, the plane bound of DESIGN.md section 4.8 holds, and the deep entry points are declared and typed."""
import os
import re

import numpy as np
import pytest

import deep
import orc

PICTURES = [(64, 48, 1, 0), (131, 77, 3, 0), (320, 240, 3, 0), (53, 37, 3, 1), (17, 300, 1, 1)]   # W, H, C, kind


def _prefixes(data):
    L = len(data)
    return sorted({L, L - 1, L // 2, L // 5, 40, 7, 6})


@pytest.mark.parametrize("pic", PICTURES)
def test_composition_equals_the_whole_file_oracle_on_8_bit_pictures(pic):
    """deep_encode == orc.encode (whole and with CAPACITY, bytes and counters) and deep_decode(..., 255) == orc.decode
    on whole streams, prefixes and PIXELS caps: the helper restates the oracle, which is pinned on the reference."""
    W, H, C, kind = pic
    pix = orc.synth(W, H, C, 3, kind)
    whole = None
    for capacity in (0, 100, 500, 3000):
        want, wst = orc.encode(pix, capacity)
        got, gst = deep.deep_encode(pix.astype(np.uint16), capacity)
        assert got == want, capacity
        assert (gst.meta_bits, gst.root_bits, gst.total_bits, list(gst.planes)) == \
            (wst.meta_bits, wst.root_bits, wst.total_bits, list(wst.planes)), capacity
        whole = whole or want
    for cut in _prefixes(whole):
        for pixels_max in (-1, 0, 2000):
            ref = orc.decode(whole[:cut], pixels_max)
            got = deep.deep_decode(whole[:cut], W, H, C, 255, pixels_max)
            assert (ref is None) == (got is None), (cut, pixels_max)
            if ref is not None:
                assert got.shape == ref.shape and (got == ref).all(), (cut, pixels_max)


def test_composition_equals_the_reference_binarys_streams():
    """tests/golden/smpte*.dwt were written by the reference's ./encode (tests/golden/make_golden.py)."""
    pix = orc.read_pnm(os.path.join(orc.GOLDEN, "smpte.pnm")).astype(np.uint16)
    for name, capacity in (("smpte.dwt", 0), ("smpte_cap100.dwt", 100), ("smpte_cap4096.dwt", 4096)):
        want = open(os.path.join(orc.GOLDEN, name), "rb").read()
        assert deep.deep_encode(pix, capacity)[0] == want, name


@pytest.mark.parametrize("M", [1023, 4095, 16383, 65535])
@pytest.mark.parametrize("C", [1, 3])
def test_deep_pictures_round_trip(M, C):
    W, H = 131, 77
    pix = deep.smooth_noise(W, H, C, M, seed=M + C)
    assert pix.max() <= M and pix.max() > M // 2
    data, st = deep.deep_encode(pix)
    back = deep.deep_decode(data, W, H, C, M)
    assert back.dtype == np.uint16 and (back == pix).all()


def test_generators_plane_counts():
    """What the GPU tests' pictures ask of the coder (256x200): the noisy ones need 13-15 planes at maxval 4095,
    ordinary 16-bit pictures fit, full-range 16-bit noise does not."""
    W, H, M = 256, 200, 4095
    planes = lambda p: list(deep.deep_encode(p)[1].planes)[:p.shape[2]]   # noqa: E731
    assert planes(deep.smooth_noise(W, H, 1, M, 1)) == [9]
    assert planes(deep.noise(W, H, 3, M, 1)) == [13, 14, 14]
    assert planes(deep.checker(W, H, 1, M)) == [13]
    assert planes(deep.checker(W, H, 3, M)) == [2, 0, 14]
    assert planes(deep.blocks(W, H, 3, M, 1)) == [13, 15, 14]
    assert max(planes(deep.smooth_noise(W, H, 3, 65535, 1))) <= 16
    assert max(planes(deep.noise(W, H, 3, 65535, 1))) > 16 and planes(deep.noise(W, H, 1, 65535, 4)) == [17]


GEOMETRIES = [(512, 512), (1031, 517), (2048, 1000), (1000, 1000), (8, 8), (9, 8), (15, 15), (16, 16), (17, 300),
              (300, 17), (8, 1000), (64, 64), (131, 77), (255, 257), (1920, 1080), (1023, 9)]


@pytest.mark.parametrize("wh", GEOMETRIES)
def test_gain_stays_below_the_16_plane_limit(wh):
    """maxval 4095 needs a gain below 65536 / 4095 = 16.0 for 16 planes, gray at maxval 8191 one below 8.0."""
    g = deep.Gain(*wh)
    assert 1.0 < g.gray < 8.0
    assert g.chroma == pytest.approx(2 * g.gray) and g.chroma < 16.0


def test_gain_of_the_documented_geometries():
    assert deep.Gain(512, 512).gray == pytest.approx(4.078, abs=1e-3)
    assert deep.Gain(1031, 517).gray == pytest.approx(4.422, abs=1e-3)
    assert deep.Gain(1000, 1000).chroma == pytest.approx(9.069, abs=1e-3)
    g = deep.Gain(2048, 1000)
    assert (g.gray, g.chroma) == (pytest.approx(4.278, abs=1e-3), pytest.approx(8.556, abs=1e-3))


def test_worst_pictures_through_the_integer_oracle():
    """The pictures the gain model calls worst, through the real (rounding) transform: 12 planes for 8-bit RGB — one
    more than an earlier comment allowed —, 15 / 16 at maxval 4095, 16 for gray at 8191; the 16-plane ones have
    coefficients in [2^15, 2^16)."""
    sq, odd = deep.Gain(512, 512), deep.Gain(1031, 517)
    for g in (sq, odd):
        assert list(deep.deep_encode(g.worst_rgb(255))[1].planes) == [2, 12, 2]
    assert max(deep.deep_encode(sq.worst_gray(255))[1].planes) <= 11
    assert list(deep.deep_encode(sq.worst_rgb(4095))[1].planes) == [2, 16, 2]
    assert list(deep.deep_encode(odd.worst_gray(4095))[1].planes)[:1] == [15]
    assert list(deep.deep_encode(odd.worst_gray(8191))[1].planes)[:1] == [16]
    assert max(deep.deep_encode(odd.worst_rgb(4095))[1].planes) == 16
    pyr = orc.forward(deep.rgb2ycocg(sq.worst_rgb(4095)))
    g = orc.geometry(512, 512)
    pyr[:g.heights[0], :g.widths[0]] = 0   # the root image
    assert 1 << 15 <= np.abs(pyr).max() < 1 << 16


DEEP_SYMBOLS = ["dwtx_planes_from_pixels16", "dwtx_pixels16_from_planes", "dwtx_transformation_fwd_pixels16",
                "dwtx_transformation_inv_pixels16", "dwtx_encode_bound16", "dwtx_encode_device16", "dwtx_decode_device16",
                "dwtx_encode_images16", "dwtx_decode_images16"]


def test_deep_entry_points_are_declared_typed_and_exported():
    from dwt_amd import _lib

    text = open(os.path.join(orc.ROOT, "include", "dwtx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in DEEP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/dwtx.h"
        assert name in _lib.SYMBOLS, f"{name} is not typed in dwt_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libdwtx.so"
    for W, H, C in ((8, 8, 1), (131, 77, 3), (4096, 4096, 1)):
        b = lib.dwtx_encode_bound16(W, H, C)
        assert b % 8 == 0 and 4 * W * H * C + 4096 <= b < 4 * W * H * C + 4096 + 8
    import dwt_amd
    for m in ("planes_from_pixels16", "pixels16_from_planes", "transformation_fwd_pixels16", "transformation_inv_pixels16",
              "encode16", "decode16", "encode_device16", "decode_device16"):
        assert callable(getattr(dwt_amd.Context, m))
