"""CPU: what tests/test_order_gpu.py rests on.  Its pictures tell the channel orders apart — R and B differ, the stream of
a picture differs from that of its channel-reversed twin, and a cut stream decodes to something that is not a plain channel
swap of the twin's — so a kernel that ignored the order, or swapped after the clamps' wrong side, could not pass; the
reversing layout writes R to memory sample 2; and the Python layer checks `order` before it touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc
import test_order_gpu as G
import test_views_gpu as V

depths = pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])


@depths
@pytest.mark.parametrize("wh", G.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_the_pictures_tell_the_orders_apart(wh, is16):
    W, H = wh
    for i in range(G.PICTURES):
        p = V.picture(W, H, 3, is16, i)
        q = np.ascontiguousarray(p[..., ::-1])
        assert (p[..., 0] != p[..., 2]).mean() >= 0.25, i
        data, st = V.oracle_encode(W, H, 3, is16, i)
        twin, tst = (V.deep.deep_encode if is16 else orc.encode)(q)
        assert data != twin, i
        a = V.oracle_decode(V.cut(data, st), W, H, 3, is16)
        b = V.oracle_decode(V.cut(twin, tst), W, H, 3, is16)
        assert a is not None and b is not None, i
        assert a.shape != b.shape or (a[..., ::-1] != b).any(), i


def test_the_tile_frame_tells_the_orders_apart():
    src = orc.synth(300, 200, 3, 5, 0)
    assert (src[..., 0] != src[..., 2]).mean() >= 0.25
    assert orc.encode(src[:128, :128])[0] != orc.encode(np.ascontiguousarray(src[:128, :128, ::-1]))[0]


@depths
def test_the_reversing_layout_writes_r_to_memory_sample_2(is16):
    W, H = 12, 9
    for kind in G.ALL:
        L, _ = G.made(kind, W, H)
        buf = V.pattern(L.samples, is16)
        before = buf.copy()
        pics = [V.deep.noise(W, H, 3, V.M16, seed=i) if is16 else orc.synth(W, H, 3, i, 1) for i in range(L.n)]
        for w, pic in zip(L.np_windows(buf), pics):
            w[...] = pic
        plain = V.Layout.np_windows(L, buf)
        for w, pic in zip(plain, pics):
            assert (w[..., 2] == pic[..., 0]).all() and (w[..., 1] == pic[..., 1]).all() and (w[..., 0] == pic[..., 2]).all(), kind
        # and nothing but the windows' three samples was written
        for w, o in zip(plain, V.Layout.np_windows(L, before)):
            o[...] = w
        assert (before == buf).all(), kind


def test_order_is_checked_in_python_before_any_device_call():
    import dwt_amd

    assert dwt_amd.view_order("rgb") == G.RGB == 0 and dwt_amd.view_order("bgr") == G.BGR == 1
    for bad in ("RGB", "bgra", "", None, 1, 0, b"bgr"):
        with pytest.raises(ValueError, match="'rgb' or as 'bgr'"):
            dwt_amd.view_order(bad)

    class NoDevice:   # every attribute a device call would need raises
        def __getattr__(self, name):
            raise AssertionError("touched %s before checking order" % name)

    for call in (dwt_amd.Context.encode_view, dwt_amd.Context.decode_view):
        with pytest.raises(ValueError, match="'rgb' or as 'bgr'"):
            call(NoDevice(), *([None] * (1 if call is dwt_amd.Context.encode_view else 3)), order="grb")


def test_the_header_and_the_loader_agree_on_the_order_calls():
    import dwt_amd
    from dwt_amd import _lib

    text = open(os.path.join(orc.ROOT, "include", "dwtx.h")).read()
    assert re.search(r"enum\s*\{\s*DWTX_ORDER_RGB\s*=\s*0\s*,\s*DWTX_ORDER_BGR\s*=\s*1\s*\}", text)
    for name, nargs in (("dwtx_encode_view_order", 11), ("dwtx_decode_view_order", 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == nargs, name
    assert C.sizeof(dwt_amd.View) == 4 * 4 + 8 + 4 * 8, "dwtx_view is frozen"
