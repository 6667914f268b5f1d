"""CPU: the host side of stepped views (dwtx_encode_view_step / dwtx_decode_view_step, include/dwtx.h) — the mapping from
a tensor's shape and strides to a view's fields and its pixel step, and the ABI the feature was built beside: dwtx_view is
what it was, the two calls are declared and typed."""
import ctypes as C
import os
import re

import pytest

import orc

ROOT = orc.ROOT
MATCH = "interleaved .* or planar"


def fields(shape, strides, stepped=False):
    import dwt_amd

    return dwt_amd.view_fields(shape, strides, stepped)


def contiguous(shape):
    s, out = 1, []
    for d in reversed(shape):
        out.append(s)
        s *= d
    return tuple(reversed(out))


def test_an_rgba_batch_gives_rgb_and_alpha_views():
    n, H, W = 5, 68, 72
    st = contiguous((n, H, W, 4))
    rgb = fields((n, H, W, 3), st, stepped=True)
    assert rgb == dict(W=W, H=H, channels=3, n=n, cols=0, row_pitch=4 * W, image_stride=4 * W * H, band_stride=0, channel_stride=0,
                       pixel_step=4)
    a = fields((n, H, W, 1), st, stepped=True)
    assert a == dict(rgb, channels=1)


def test_nv12_chroma_and_bayer_planes():
    H, W = 68, 72
    uv = fields((1, H, W, 1), (0, 2 * W, 2, 1), stepped=True)           # uv[:, :, 0::2] of an interleaved [H, 2W] chroma plane
    assert (uv["pixel_step"], uv["row_pitch"], uv["channels"]) == (2, 2 * W, 1)
    bayer = fields((1, H, W, 1), (0, 4 * W, 2, 1), stepped=True)        # mosaic[dy::2, dx::2] of a [2H, 2W] frame
    assert (bayer["pixel_step"], bayer["row_pitch"]) == (2, 4 * W)


def test_a_tile_grid_of_an_rgba_frame():
    rows, cols, H, W, FW = 2, 3, 64, 128, 400
    f = fields((rows, cols, H, W, 3), (H * FW * 4, W * 4, FW * 4, 4, 1), stepped=True)
    assert f == dict(W=W, H=H, channels=3, n=6, cols=3, row_pitch=FW * 4, image_stride=W * 4, band_stride=H * FW * 4, channel_stride=0,
                     pixel_step=4)


@pytest.mark.parametrize("stepped", [False, True])
def test_dense_and_planar_tensors_map_as_before(stepped):
    n, H, W = 4, 68, 72
    assert fields((n, H, W, 3), contiguous((n, H, W, 3)), stepped) == dict(
        W=W, H=H, channels=3, n=n, cols=0, row_pitch=3 * W, image_stride=3 * W * H, band_stride=0, channel_stride=0, pixel_step=0)
    assert fields((n, H, W, 1), contiguous((n, H, W, 1)), stepped)["pixel_step"] == 0
    nchw = contiguous((n, 3, H, W))
    p = fields((n, H, W, 3), (nchw[0], nchw[2], nchw[3], nchw[1]), stepped)      # permute(0, 2, 3, 1)
    assert (p["channel_stride"], p["pixel_step"], p["row_pitch"], p["image_stride"]) == (H * W, 0, W, 3 * H * W)


def test_what_is_refused():
    n, H, W = 2, 68, 72
    st6 = contiguous((n, H, W, 6))
    rgba = contiguous((n, H, W, 4))
    # without the keyword: every stepped tensor, with the message there was
    for shape, strides in (((n, H, W, 3), rgba), ((n, H, W, 1), rgba), ((n, H, W // 2, 3), (st6[0], st6[1], 12, 1))):
        with pytest.raises(ValueError, match=MATCH):
            fields(shape, strides)
    # with it: still no channel stride of 2, no two channels, no step below the channels, no broadcast columns
    for shape, strides in (((n, H, W, 3), (st6[0], st6[1], 6, 2)), ((n, H, W, 2), st6), ((n, H, W, 3), (rgba[0], rgba[1], 2, 1)),
                           ((n, H, W, 1), (rgba[0], rgba[1], 0, 1))):
        with pytest.raises(ValueError, match=MATCH):
            fields(shape, strides, stepped=True)
    with pytest.raises(ValueError):
        fields((H, W, 3), (3 * W, 3, 1), stepped=True)


def test_the_view_struct_is_what_it_was():
    import dwt_amd

    assert C.sizeof(dwt_amd.View) == 56
    assert [f[0] for f in dwt_amd.View._fields_][-1] == "channel_stride"
    assert len(dwt_amd.View._fields_) == 9


def test_the_two_calls_are_declared_and_typed():
    from dwt_amd import _lib

    text = open(os.path.join(ROOT, "include", "dwtx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    enc = re.search(r"int\s+dwtx_encode_view_step\s*\(([^)]*)\)", text).group(1)
    dec = re.search(r"int\s+dwtx_decode_view_step\s*\(([^)]*)\)", text).group(1)
    assert [a.split()[-1].lstrip("*") for a in enc.split(",")] == ["ctx", "src", "pixel_step", "W", "H", "n", "capacity", "dev_out", "out_stride",
                                                                   "dev_info"]
    assert [a.split()[-1].lstrip("*") for a in dec.split(",")] == ["ctx", "dev_streams", "stream_stride", "dev_lens", "W", "H", "n", "levels_max",
                                                                   "dst", "pixel_step", "host_info"]
    for name, nargs, step_at in (("dwtx_encode_view_step", 10, 2), ("dwtx_decode_view_step", 11, 9)):
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == nargs and args[step_at] is C.c_size_t
        assert hasattr(_lib.load(), name)
    # the struct in the header is untouched too: channel_stride is its last member
    body = re.search(r"typedef struct dwtx_view\s*\{(.*?)\}\s*dwtx_view;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == ["dev", "sample_bytes", "channels", "maxval", "cols", "row_pitch", "image_stride", "band_stride",
                                              "channel_stride"]
