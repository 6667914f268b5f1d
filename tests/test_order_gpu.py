"""GPU: views whose three channels lie as B, G, R — dwtx_encode_view_order / dwtx_decode_view_order (include/dwtx.h): BGRA
and BGRX surfaces, OpenCV-style BGR frames and planar B, G, R planes, coded where they lie.

The yardstick is that of tests/test_views_gpu.py, whose helpers this file uses unchanged: the oracle on the dense crop —
here with its last axis reversed, i.e. on the R, G, B picture whose colours the window holds the other way round — exact,
and for a decode every sample of a pattern-prefilled buffer, which is what shows that the fourth bytes and the frame around
the windows are untouched.  A BGR layout is a Layout whose numpy windows are channel-reversed views (numpy allows the
negative stride torch refuses): what the helpers write as R lands in memory sample 2, or in the third plane.
tests/test_order_cpu.py shows that the pictures used here tell the orders apart."""
import ctypes as C

import numpy as np
import pytest

import orc
import test_planar_gpu as P
import test_step_gpu as S
import test_views_gpu as V
from test_views_gpu import Layout

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
RGB, BGR = 0, 1

# V.SHAPES: 256x256, 132x100, 72x68 wide (and the two-levels-per-pass inverse), 64x64 the LDS tail, 8x8 the minimum, 37x53 and
# 130x67 the general path; 264x68: 66 quads, so the second wave strip ends inside the row — lane 63's right neighbour of the
# first strip and lane 0's left neighbours of the second come from the edge words, where a missed swap shows in a few columns
SHAPES = V.SHAPES + [(264, 68)]
shapes = pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
depths = pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
PICTURES = 12   # the most windows a layout here has (a 3 x 4 grid), pictures 0 .. 11


class Reversed(Layout):
    """A layout whose windows lie as B, G, R: the numpy windows are handed out channel-reversed."""

    def np_windows(self, buf):
        return [w[..., ::-1] for w in Layout.np_windows(self, buf)]


def bgr(L):
    return Reversed(L.samples, L.off, L.shape, L.strides)


class Bgr:
    """The context with order="bgr" on its two view calls (and stepped, where the layout has a step): what V.check_encode /
    V.check_decode call.  check_encode also compares with encode_device of the view's dense copy, which lies as B, G, R:
    that copy is reversed before it is encoded."""

    def __init__(self, ctx, stepped):
        self._ctx, self._stepped = ctx, stepped

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def encode_view(self, t, capacity=0, **kw):
        return self._ctx.encode_view(t, capacity, stepped=self._stepped, order="bgr", **kw)

    def decode_view(self, streams, lens, into, **kw):
        return self._ctx.decode_view(streams, lens, into, stepped=self._stepped, order="bgr", **kw)

    def encode_device(self, pix, capacity=0, **kw):
        return self._ctx.encode_device(pix.flip(-1).contiguous(), capacity, **kw)

    def encode_device16(self, pix, capacity=0, **kw):
        return self._ctx.encode_device16(pix.flip(-1).contiguous(), capacity, **kw)


# kind -> (layout maker of (W, H), stepped).  dense: 3-sample pixels; step4: 4-sample pixels on the 4-sample grid (BGRA8: the
# wide kernels for 4-byte pixels; BGRA16: the general path)
KINDS = {
    "dense-stack": (lambda W, H: V.stack(W, H, 3), False),
    "dense-band": (lambda W, H: V.band(W, H, 3), False),
    "dense-grid": (lambda W, H: V.grid(W, H, 3), False),
    "step4-stack": (lambda W, H: S.sstack(W, H, 3, 4), True),
    "step4-band": (lambda W, H: S.sband(W, H, 3, 4), True),
    "step4-grid": (lambda W, H: S.sgrid(W, H, 3, 4), True),
}
# one layout each: ABGR (4-sample pixels one sample off the grid, at dev + 1: the general path), step 5, and planar B, G, R
# planes — an NCHW stack and the tile grid of a CHW frame
OTHERS = {
    "abgr": (lambda W, H: S.sgrid(W, H, 3, 4, off=1), True),
    "step5": (lambda W, H: S.sgrid(W, H, 3, 5), True),
    "nchw": (lambda W, H: P.nchw(W, H), False),
    "chw_grid": (lambda W, H: P.chw_grid(W, H), False),
}
ALL = {**KINDS, **OTHERS}


def made(kind, W, H):
    make, stepped = ALL[kind]
    return bgr(make(W, H)), stepped


def test_the_layouts_are_what_they_claim():
    for kind, is16, (W, H) in SWITCH_CASES:   # on the quad grid: what dwtx_pixels::wide() asks (8 bytes of deep samples are 4 samples)
        L, _ = made(kind, W, H)
        assert W % 4 == 0 and L.off % 4 == 0 and all(s % 4 == 0 for s in L.strides[:-2]), kind
    for kind in ALL:
        L, _ = made(kind, 72, 68)
        assert L.n <= PICTURES
        buf = np.zeros(L.samples, dtype=np.uint8)
        for w in L.np_windows(buf):
            w[..., 0] = 1   # "R"
        plain = Layout.np_windows(L, buf)
        assert all((w[..., 2] == 1).all() and (w[..., :2] == 0).all() for w in plain), kind
    L, _ = made("step4-grid", 72, 68)
    assert L.off % 4 == 0 and all(s % 4 == 0 for s in L.strides[:-1])
    L, _ = made("abgr", 72, 68)
    assert L.off % 4 == 1 and L.strides[-2] == 4
    assert made("step5", 72, 68)[0].strides[-2] == 5
    assert made("nchw", 72, 68)[0].strides[-2] == 1 and made("chw_grid", 72, 68)[0].strides[-2] == 1


# ---- encode, decode ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
@depths
@shapes
def test_bgr_encode_equals_the_oracle_on_the_reversed_crops(ctx, wh, is16, kind):
    W, H = wh
    L, stepped = made(kind, W, H)
    V.check_encode(Bgr(ctx, stepped), L, W, H, 3, is16)   # capacities 0 and 500


@pytest.mark.parametrize("kind", list(KINDS))
@depths
@shapes
def test_bgr_decode_writes_the_colours_swapped_and_nothing_else(ctx, wh, is16, kind):
    W, H = wh
    L, stepped = made(kind, W, H)
    for name, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n):   # whole, cut, mixed, capped
        print(name)
        V.check_decode(Bgr(ctx, stepped), L, W, H, 3, is16, rows, pixels_max)


@pytest.mark.parametrize("kind", list(OTHERS))
@depths
@shapes
def test_bgr_off_the_grid_with_step_5_and_planar(ctx, wh, is16, kind):
    W, H = wh
    L, stepped = made(kind, W, H)
    b = Bgr(ctx, stepped)
    V.check_encode(b, L, W, H, 3, is16, capacities=(0,))
    for name, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n):
        print(name)
        V.check_decode(b, L, W, H, 3, is16, rows, pixels_max)


# ---- one BGRA surface, two streams, two contexts ---------------------------------------------------------------------------

def test_a_bgra_surface_round_trips_as_bgr_and_alpha():
    import torch

    import dwt_amd

    W, H, n = 132, 100, 3
    src = np.empty((n, H, W, 4), dtype=np.uint8)
    for i in range(n):
        src[i, ..., 2::-1] = V.picture(W, H, 3, False, i)   # memory: B, G, R
        src[i, ..., 3] = V.picture(W, H, 1, False, i + 1)[..., 0]
    dev = torch.device("cuda", 0)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    c1, c2 = dwt_amd.Context(0, stream=s1.cuda_stream), dwt_amd.Context(0, stream=s2.cuda_stream)
    try:
        bgra = torch.from_numpy(src).to(dev)
        pat = V.pattern(src.size, False).reshape(src.shape)
        back = torch.from_numpy(pat).to(dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            c_s, c_i = c1.encode_view(bgra[..., :3], stepped=True, order="bgr")
        with torch.cuda.stream(s2):
            a_s, a_i = c2.encode_view(bgra[..., 3:], stepped=True, order="bgr")   # (gray: the order is ignored)
        s1.synchronize()
        s2.synchronize()
        host, ahost = c_s.cpu().numpy(), a_s.cpu().numpy()
        for i, (I, A) in enumerate(zip(V.infos_of(c_i), V.infos_of(a_i))):
            assert host[i, :I.nbytes].tobytes() == V.oracle_encode(W, H, 3, False, i)[0], i
            assert ahost[i, :A.nbytes].tobytes() == V.oracle_encode(W, H, 1, False, i + 1)[0], i
        with torch.cuda.stream(s1):
            c1.decode_view(c_s, c1.stream_lengths(c_i), back[..., :3], stepped=True, order="bgr")
        s1.synchronize()
        got = back.cpu().numpy()
        assert (got[..., 3] == pat[..., 3]).all(), "the BGR decode wrote alpha bytes"
        assert (got[..., :3] == src[..., :3]).all()
        with torch.cuda.stream(s2):
            c2.decode_view(a_s, c2.stream_lengths(a_i), back[..., 3:], stepped=True)
        s2.synchronize()
        assert (back.cpu().numpy() == src).all(), "the surface is not the source in every byte"
    finally:
        c1.close()
        c2.close()


# ---- DWTX_ORDER_RGB is the step call ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dense-grid", "step4-grid", "nchw"])
def test_order_rgb_is_the_step_call(ctx, kind):
    import torch

    import dwt_amd

    W, H = 132, 100
    L = ALL[kind][0](W, H)   # (not reversed: R, G, B as it lies)
    n = L.n
    buf = V.pattern(L.samples, False)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = V.picture(W, H, 3, False, i)
    tbuf = V.to_device(ctx, buf)
    f = dwt_amd.view_fields(L.shape, L.strides, True)
    stride = ctx.lib.dwtx_encode_bound(W, H, 3)

    def view(t):
        return dwt_amd.View(t.data_ptr() + L.off, 1, 3, 255, f["cols"], f["row_pitch"], f["image_stride"], f["band_stride"], f["channel_stride"])

    def encode(order):
        out = torch.zeros((n, stride), dtype=torch.uint8, device=ctx.device)
        info = torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
        v = view(tbuf)
        if order is None:
            rc = ctx.lib.dwtx_encode_view_step(ctx.h, C.byref(v), f["pixel_step"], W, H, n, 0, out.data_ptr(), stride, info.data_ptr())
        else:
            rc = ctx.lib.dwtx_encode_view_order(ctx.h, C.byref(v), f["pixel_step"], order, W, H, n, 0, out.data_ptr(), stride, info.data_ptr())
        assert rc == 0, order
        ctx.sync()
        return out, info

    plain, pinfo = encode(None)
    for i, I in enumerate(V.infos_of(pinfo)):
        assert plain[i, :I.nbytes].cpu().numpy().tobytes() == V.oracle_encode(W, H, 3, False, i)[0], i
    out, info = encode(RGB)
    assert torch.equal(out, plain) and [V.fields(I) for I in V.infos_of(info)] == [V.fields(I) for I in V.infos_of(pinfo)]
    swapped, _ = encode(BGR)
    assert not torch.equal(swapped, plain), "the order made no difference to the streams"
    lens = ctx.stream_lengths(pinfo)
    infos = (dwt_amd.DecodeInfo * n)()

    def decode(order):
        back = V.to_device(ctx, V.pattern(L.samples, False))
        v = view(back)
        if order is None:
            rc = ctx.lib.dwtx_decode_view_step(ctx.h, plain.data_ptr(), stride, lens.data_ptr(), W, H, n, -1, C.byref(v), f["pixel_step"],
                                               C.cast(infos, C.c_void_p))
        else:
            rc = ctx.lib.dwtx_decode_view_order(ctx.h, plain.data_ptr(), stride, lens.data_ptr(), W, H, n, -1, C.byref(v), f["pixel_step"],
                                                order, C.cast(infos, C.c_void_p))
        assert rc == 0, order
        ctx.sync()
        return back

    want = decode(None)
    assert torch.equal(want, tbuf)
    assert torch.equal(decode(RGB), want)


# ---- the codec's other paths -----------------------------------------------------------------------------------------------

SWITCHES = ["no_fused_levels", "no_fine16", "no_pixels16"]
# wide layouts (V.stack's pitch is off the quad grid, so the dense ones are grids): 256x256 also takes the two-level inverse
SWITCH_CASES = [("dense-grid", False, (256, 256)), ("step4-stack", False, (256, 256)), ("dense-grid", True, (132, 100))]


@pytest.mark.parametrize("kind,is16,wh", SWITCH_CASES, ids=["bgr8", "bgra8", "bgr16"])
@pytest.mark.parametrize("name", SWITCHES)
def test_bgr_under_the_switches(ctx, opts, name, kind, is16, wh):
    """The paths the diagnostic switches choose between — one level at a time, int32 rings, deep pixels through the general
    conversions — agree on B, G, R pixels too."""
    W, H = wh
    opts.set(name, 1)
    L, stepped = made(kind, W, H)
    b = Bgr(ctx, stepped)
    V.check_encode(b, L, W, H, 3, is16, capacities=(0,))
    for case, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n)[::2]:   # whole, mixed
        print(case)
        V.check_decode(b, L, W, H, 3, is16, rows, pixels_max)


# ---- parts: a part starts mid-grid and must keep the order -----------------------------------------------------------------

def test_bgr_encoder_parts_start_mid_grid(ctx, opts):
    """128 windows, which the encoder cuts into parts, each starting at a window of its own of the 16 x 8 grid (part_images, the
    host pipelines' part size, is set as well and changes nothing here)."""
    W, H = 72, 68
    opts.set("part_images", 8)
    L = bgr(S.sgrid(W, H, 3, 4, rows=8, cols=16))
    V.check_encode(Bgr(ctx, True), L, W, H, 3, False, capacities=(0,))


@pytest.mark.parametrize("kind", ["step4-grid", "chw_grid"])
def test_bgr_decoder_parts_start_mid_grid(ctx, opts, kind):
    W, H = 72, 68
    opts.set("decode_parts", 2)
    L, stepped = made(kind, W, H)
    for name, rows, pixels_max in V.decode_cases(W, H, 3, False, L.n)[::2]:
        V.check_decode(Bgr(ctx, stepped), L, W, H, 3, False, rows, pixels_max)


# ---- frames as tiles -------------------------------------------------------------------------------------------------------

def test_a_bgra_frame_round_trips_through_tiles(ctx):
    import torch

    from dwt_amd import tiles

    FW, FH, tile = 300, 200, 128   # all four tile groups
    src = orc.synth(FW, FH, 3, 5, 0)
    pat = V.pattern(FW * FH * 4, False).reshape(FH, FW, 4)
    surface = pat.copy()
    surface[..., 2::-1] = src
    bgra = torch.from_numpy(surface).to(ctx.device)
    coded = tiles.encode_frame(ctx, bgra[..., :3], tile, stepped=True, order="bgr")
    assert len(coded) == 4
    for g, streams, lens, info in coded:
        host, ln = streams.cpu().numpy(), lens.cpu().numpy()
        for i in range(g.cols * g.rows):
            x, y = g.x0 + (i % g.cols) * g.W, g.y0 + (i // g.cols) * g.H
            want, st = orc.encode(src[y:y + g.H, x:x + g.W])
            assert host[i, :ln[i]].tobytes() == want, (g.x0, g.y0, i)
    back = torch.from_numpy(pat).to(ctx.device)
    tiles.decode_frame(ctx, coded, into=back[..., :3], stepped=True, order="bgr")
    assert (back.cpu().numpy() == surface).all(), "the surface is not the source in every byte"


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_bad_orders_are_refused_and_nothing_is_written(ctx):
    import torch

    import dwt_amd

    W, H, n, St = 72, 68, 4, 4
    FW = (4 * W + 8) * St
    pat = V.pattern((2 * H + 8) * FW + 64, False)
    tbuf = V.to_device(ctx, pat)
    data, _ = V.oracle_encode(W, H, 3, False, 0)
    stride = (len(data) + 64 + 7) // 8 * 8
    host = np.zeros((n, stride), dtype=np.uint8)
    host[:, :len(data)] = np.frombuffer(data, dtype=np.uint8)
    streams = torch.from_numpy(host).to(ctx.device)
    lens = torch.full((n,), len(data), dtype=torch.int64, device=ctx.device)
    out_pat = V.pattern(n * 3 * 8192, False).reshape(n, 3 * 8192)
    info_pat = V.pattern(n * C.sizeof(dwt_amd.StreamInfo), False).reshape(n, -1)
    out, info = torch.from_numpy(out_pat).to(ctx.device), torch.from_numpy(info_pat).to(ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()
    good = dwt_amd.View(tbuf.data_ptr(), 1, 3, 255, 0, FW, W * St, 0, 0)
    planar = dwt_amd.View(tbuf.data_ptr(), 1, 3, 255, 0, W + 8, 3 * H * (W + 8), 0, H * (W + 8))

    def decode(v, step, order):
        return ctx.lib.dwtx_decode_view_order(ctx.h, streams.data_ptr(), stride, lens.data_ptr(), W, H, n, -1, C.byref(v), step, order,
                                              C.cast(infos, C.c_void_p))

    def encode(v, step, order):
        return ctx.lib.dwtx_encode_view_order(ctx.h, C.byref(v), step, order, W, H, n, 0, out.data_ptr(), out.shape[1], info.data_ptr())

    bad = {"order 2": (good, St, 2), "order -1": (good, St, -1), "planar B, G, R with a step": (planar, St, BGR)}
    for name, (v, step, order) in bad.items():
        for call in (decode, encode):
            assert call(v, step, order) == ERR_ARG, name
            assert ctx.lib.dwtx_last_error(), name
    ctx.sync()
    assert (tbuf.cpu().numpy() == pat).all(), "a refused view was written to"
    assert (out.cpu().numpy() == out_pat).all() and (info.cpu().numpy() == info_pat).all(), "a refused encode wrote streams"
    # the same views with an order the header names, and the planar one without its step, are taken
    assert decode(good, St, BGR) == 0 and encode(good, St, BGR) == 0
    assert decode(planar, 0, BGR) == 0 and encode(planar, 0, BGR) == 0
    ctx.sync()
    with pytest.raises(ValueError, match="'rgb' or as 'bgr'"):
        ctx.encode_view(tbuf[:n * H * W * 3].view(n, H, W, 3), order="rgba")
    with pytest.raises(ValueError, match="'rgb' or as 'bgr'"):
        ctx.decode_view(streams, lens, tbuf[:n * H * W * 3].view(n, H, W, 3), order=1)
