"""GPU: views whose pixels lie further apart than their own samples — dwtx_encode_view_step / dwtx_decode_view_step
(include/dwtx.h): the RGB and the alpha of an RGBA surface, the chroma planes of NV12, the planes of a Bayer mosaic, coded
where they lie.

The yardstick is that of tests/test_views_gpu.py, whose helpers this file uses: the oracle on the dense interleaved crop,
exact, and for a decode every sample of a pattern-prefilled buffer — which is what shows that the samples between the
pixels (the fourth byte) and the frame around the windows are untouched.  A stepped layout is a Layout like any other:
shape [n,H,W,C] or [bands,cols,H,W,C] whose column stride is the pixel step."""
import ctypes as C

import numpy as np
import pytest

import orc
import test_views_gpu as V
from test_views_gpu import Layout, MY

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG


class Stepped:
    """The context with stepped=True on its two view calls: what V.check_encode / V.check_decode call."""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def encode_view(self, t, capacity=0, **kw):
        return self._ctx.encode_view(t, capacity, stepped=True, **kw)

    def decode_view(self, streams, lens, into, **kw):
        return self._ctx.decode_view(streams, lens, into, stepped=True, **kw)


@pytest.fixture
def sctx(ctx):
    return Stepped(ctx)


# ---- layouts.  S: the pixel step in samples.  With S = 4 and nothing else said, the origin, the pitch and every stride are
# multiples of 4 samples (what the wide kernels for 8-bit RGB in 4-byte pixels ask); off: samples added to the origin; pad: samples added to a
# frame row; pm: the row pitch in frame rows (2: every other row, a Bayer plane)

def sstack(W, H, Cn, S, n=3):
    pitch = W * S + 8
    slot = H * pitch + 12
    return Layout(4 + n * slot, 4, (n, H, W, Cn), (slot, pitch, S, 1))


def sband(W, H, Cn, S):
    FW = (4 * W + 8) * S
    return Layout((H + 2 * MY) * FW, MY * FW + 4 * S, (4, H, W, Cn), (W * S, FW, S, 1))


def sgrid(W, H, Cn, S, off=0, pad=0, pm=1, rows=3, cols=4):
    FW = (cols * W + 8) * S + pad
    return Layout((rows * H * pm + 2 * MY) * FW, MY * FW + 4 * S + off, (rows, cols, H, W, Cn), (H * pm * FW, W * S, pm * FW, S, 1))


LAYOUTS = {"stack": sstack, "band": sband, "grid": sgrid}
depths = pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
shapes = pytest.mark.parametrize("wh", V.SHAPES, ids=lambda wh: "%dx%d" % wh)
wide_shapes = pytest.mark.parametrize("wh", V.WIDE, ids=lambda wh: "%dx%d" % wh)
CLASSES = [(132, 100), (64, 64), (37, 53)]   # wide, tail, general
class_shapes = pytest.mark.parametrize("wh", CLASSES, ids=lambda wh: "%dx%d" % wh)


def test_the_step4_layouts_are_on_the_4_byte_grid():
    for make in LAYOUTS.values():
        L = make(72, 68, 3, 4)
        assert L.off % 4 == 0 and all(s % 4 == 0 for s in L.strides[:-1]) and L.strides[-2:] == (4, 1), L.strides


def check_both(sctx, L, W, H, Cn, is16, capacities=(0,), cases=slice(None, None, 2)):
    V.check_encode(sctx, L, W, H, Cn, is16, capacities=capacities)
    for name, rows, pixels_max in V.decode_cases(W, H, Cn, is16, L.n)[cases]:
        print(name)
        V.check_decode(sctx, L, W, H, Cn, is16, rows, pixels_max)


# ---- RGB in 4-sample pixels ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(LAYOUTS))
@depths
@shapes
def test_step4_rgb_encode_equals_oracle_on_the_dense_crops(sctx, wh, is16, layout):
    W, H = wh
    V.check_encode(sctx, LAYOUTS[layout](W, H, 3, 4), W, H, 3, is16)   # capacities 0 and 500; the oracle and encode_device of the copy


@pytest.mark.parametrize("layout", list(LAYOUTS))
@depths
@shapes
def test_step4_rgb_decode_writes_the_three_samples_and_nothing_else(sctx, wh, is16, layout):
    W, H = wh
    L = LAYOUTS[layout](W, H, 3, 4)
    for name, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n):   # whole, cut, mixed, capped
        print(name)
        V.check_decode(sctx, L, W, H, 3, is16, rows, pixels_max)


@pytest.mark.parametrize("variant", ["origin+1", "pitch+1", "step5"])
@wide_shapes
def test_wide_shapes_off_the_4_byte_grid(sctx, wh, variant):
    """8-bit RGB of wide shapes whose origin is one byte off, whose pitch is no multiple of 4, or whose step is 5: the
    general path, the same bytes."""
    W, H = wh
    L = {"origin+1": lambda: sgrid(W, H, 3, 4, off=1), "pitch+1": lambda: sgrid(W, H, 3, 4, pad=1), "step5": lambda: sgrid(W, H, 3, 5)}[variant]()
    assert {"origin+1": L.off % 4 == 1, "pitch+1": L.strides[-3] % 4 == 1, "step5": L.strides[-2] == 5}[variant]
    check_both(sctx, L, W, H, 3, False)


# ---- gray with a step ---------------------------------------------------------------------------------------------------

@depths
@class_shapes
def test_alpha_of_an_rgba_grid(sctx, wh, is16):
    W, H = wh
    check_both(sctx, sgrid(W, H, 1, 4, off=3), W, H, 1, is16)


@pytest.mark.parametrize("origin", [0, 1], ids=["u", "v"])
@depths
@class_shapes
def test_nv12_chroma_planes(sctx, wh, is16, origin):
    W, H = wh
    check_both(sctx, sgrid(W, H, 1, 2, off=origin), W, H, 1, is16)


@pytest.mark.parametrize("dy,dx", [(0, 0), (0, 1), (1, 0), (1, 1)])
@depths
@class_shapes
def test_bayer_planes(sctx, wh, is16, dy, dx):
    """A plane of a mosaic: every other sample of every other row — column step 2, twice the frame's row pitch."""
    W, H = wh
    L0 = sgrid(W, H, 1, 2, pm=2)
    FW = L0.strides[-3] // 2
    L = Layout(L0.samples, L0.off + dy * FW + dx, L0.shape, L0.strides)
    check_both(sctx, L, W, H, 1, is16)


# ---- one RGBA surface, two streams ---------------------------------------------------------------------------------------

def test_an_rgba_surface_round_trips_as_rgb_and_alpha(ctx):
    import torch

    W, H, n = 132, 100, 3
    src = np.empty((n, H, W, 4), dtype=np.uint8)
    for i in range(n):
        src[i, ..., :3] = V.picture(W, H, 3, False, i)
        src[i, ..., 3] = V.picture(W, H, 1, False, i + 1)[..., 0]
    rgba = torch.from_numpy(src).to(ctx.device)
    rgb_s, rgb_i = ctx.encode_view(rgba[..., :3], stepped=True)
    a_s, a_i = ctx.encode_view(rgba[..., 3:], stepped=True)
    host, ahost = rgb_s.cpu().numpy(), a_s.cpu().numpy()
    for i, (I, A) in enumerate(zip(V.infos_of(rgb_i), V.infos_of(a_i))):
        assert host[i, :I.nbytes].tobytes() == V.oracle_encode(W, H, 3, False, i)[0], i
        assert ahost[i, :A.nbytes].tobytes() == V.oracle_encode(W, H, 1, False, i + 1)[0], i
    pat = V.pattern(src.size, False).reshape(src.shape)
    back = torch.from_numpy(pat).to(ctx.device)
    ctx.decode_view(rgb_s, ctx.stream_lengths(rgb_i), back[..., :3], stepped=True)
    got = back.cpu().numpy()
    assert (got[..., 3] == pat[..., 3]).all(), "the RGB decode wrote alpha bytes"
    assert (got[..., :3] == src[..., :3]).all()
    ctx.decode_view(a_s, ctx.stream_lengths(a_i), back[..., 3:], stepped=True)
    assert (back.cpu().numpy() == src).all(), "the surface is not the source in every byte"


# ---- the diagnostic switches ---------------------------------------------------------------------------------------------

SWITCHES = [("no_fused_levels", 1), ("no_fine16", 1), ("no_square_tiles", 1), ("lift_rows", 4), ("lift_rows", 64)]


@pytest.mark.parametrize("name,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
@wide_shapes
def test_step4_rgb_under_the_switches(sctx, opts, wh, name, value):
    """The code paths the diagnostic switches choose between agree on 4-byte pixels too."""
    W, H = wh
    opts.set(name, value)
    check_both(sctx, sstack(W, H, 3, 4), W, H, 3, False)


@pytest.mark.parametrize("rows", [16, 64])
@pytest.mark.parametrize("wh", [(128, 130), (260, 131), (68, 514)], ids=lambda wh: "%dx%d" % wh)
def test_step4_rgb_rows_per_wave_at_the_strip_edges(sctx, opts, wh, rows):
    """The 4-byte RGB surface at the strip-edge shapes of tests/test_planar_gpu.py: histograms on the finest level (128
    wide), one lane into a second strip (260), a last row pair without its odd row and strips of one row pair (131, 514)."""
    W, H = wh
    opts.set("lift_rows", rows)
    V.check_encode(sctx, sstack(W, H, 3, 4), W, H, 3, False, capacities=(0,))


# ---- parts ---------------------------------------------------------------------------------------------------------------

def test_step4_encoder_parts_start_mid_grid(sctx):
    """128 windows: the encoder's parts each start at a window of their own of the 16 x 8 grid."""
    W, H = 72, 68
    V.check_encode(sctx, sgrid(W, H, 3, 4, rows=8, cols=16), W, H, 3, False, capacities=(0,))


@pytest.mark.parametrize("parts", [2, 4])
def test_step4_decoder_parts_start_mid_grid(sctx, opts, parts):
    W, H = 72, 68
    opts.set("decode_parts", parts)
    L = sgrid(W, H, 3, 4, rows=2)
    for name, rows, pixels_max in V.decode_cases(W, H, 3, False, L.n)[::2]:
        V.check_decode(sctx, L, W, H, 3, False, rows, pixels_max)


# ---- the dense case is the plain call ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_step_zero_and_step_channels_are_the_plain_calls(ctx, Cn):
    import torch

    import dwt_amd

    W, H = 132, 100
    L = V.grid(W, H, Cn)
    n = L.n
    buf = V.pattern(L.samples, False)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = V.picture(W, H, Cn, False, i)
    tbuf = V.to_device(ctx, buf)
    bs, cols = L.strides[0], L.shape[1]
    stride = ctx.lib.dwtx_encode_bound(W, H, Cn)

    def view(t):
        return dwt_amd.View(t.data_ptr() + L.off, 1, Cn, 255, cols, L.strides[2], L.strides[1], bs)

    def encode(step):
        out = torch.zeros((n, stride), dtype=torch.uint8, device=ctx.device)
        info = torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
        v = view(tbuf)
        if step is None:
            rc = ctx.lib.dwtx_encode_view(ctx.h, C.byref(v), W, H, n, 0, out.data_ptr(), stride, info.data_ptr())
        else:
            rc = ctx.lib.dwtx_encode_view_step(ctx.h, C.byref(v), step, W, H, n, 0, out.data_ptr(), stride, info.data_ptr())
        assert rc == 0, step
        ctx.sync()
        return out, info

    plain, pinfo = encode(None)
    for i, I in enumerate(V.infos_of(pinfo)):
        assert plain[i, :I.nbytes].cpu().numpy().tobytes() == V.oracle_encode(W, H, Cn, False, i)[0], i
    lens = ctx.stream_lengths(pinfo)
    infos = (dwt_amd.DecodeInfo * n)()

    def decode(step):
        back = V.to_device(ctx, V.pattern(L.samples, False))
        v = view(back)
        if step is None:
            rc = ctx.lib.dwtx_decode_view(ctx.h, plain.data_ptr(), stride, lens.data_ptr(), W, H, n, -1, C.byref(v), C.cast(infos, C.c_void_p))
        else:
            rc = ctx.lib.dwtx_decode_view_step(ctx.h, plain.data_ptr(), stride, lens.data_ptr(), W, H, n, -1, C.byref(v), step,
                                               C.cast(infos, C.c_void_p))
        assert rc == 0, step
        ctx.sync()
        return back

    want = decode(None)
    assert torch.equal(want, tbuf)
    for step in (0, Cn):
        out, info = encode(step)
        assert torch.equal(out, plain) and [V.fields(I) for I in V.infos_of(info)] == [V.fields(I) for I in V.infos_of(pinfo)], step
        assert torch.equal(decode(step), want), step


# ---- argument rules, through ctypes -------------------------------------------------------------------------------------

def test_bad_stepped_views_are_refused_and_nothing_is_written(ctx):
    import torch

    import dwt_amd

    W, H, n, S = 72, 68, 4, 4
    row = (W - 1) * S + 3                 # a window's row: from its first sample to behind its last
    FW = (4 * W + 8) * S                  # a frame that holds four windows side by side
    win = (H - 1) * FW + row
    pat = V.pattern((2 * H + 8) * FW + 64, False)
    tbuf = V.to_device(ctx, pat)
    data, _ = V.oracle_encode(W, H, 3, False, 0)
    stride = (len(data) + 64 + 7) // 8 * 8
    host = np.zeros((n, stride), dtype=np.uint8)
    host[:, :len(data)] = np.frombuffer(data, dtype=np.uint8)
    streams = torch.from_numpy(host).to(ctx.device)
    lens = torch.full((n,), len(data), dtype=torch.int64, device=ctx.device)
    out = torch.zeros((n, 3 * 8192), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()

    def view(cols=0, pitch=FW, istride=W * S, bstride=0, cs=0):
        return dwt_amd.View(tbuf.data_ptr(), 1, 3, 255, cols, pitch, istride, bstride, cs)

    def decode(v, step=S):
        return ctx.lib.dwtx_decode_view_step(ctx.h, streams.data_ptr(), stride, lens.data_ptr(), W, H, n, -1, C.byref(v), step,
                                             C.cast(infos, C.c_void_p))

    def encode(v, step=S):
        return ctx.lib.dwtx_encode_view_step(ctx.h, C.byref(v), step, W, H, n, 0, out.data_ptr(), out.shape[1], info.data_ptr())

    bad_both = {
        "step below channels": (view(), 2),
        "planar with a step": (view(pitch=W + 8, istride=3 * H * (W + 8), cs=H * (W + 8)), S),
        "row_pitch one below a row": (view(pitch=row - 1), S),
    }
    bad_decode = {
        "stacked, windows one sample too close": (view(pitch=row, istride=(H - 1) * row + row - 1), S),
        "side by side, windows one sample too close": (view(istride=row - 1), S),
        "side by side, pitch one sample short of the band": (view(pitch=3 * row + row - 1, istride=row), S),
        "bands one sample too close": (view(cols=2, bstride=W * S + win - 1), S),
    }
    for name, (v, step) in {**bad_both, **bad_decode}.items():
        assert decode(v, step) == ERR_ARG, name
        assert ctx.lib.dwtx_last_error(), name
    for name, (v, step) in bad_both.items():
        assert encode(v, step) == ERR_ARG, name
        assert ctx.lib.dwtx_last_error(), name
    ctx.sync()
    assert (tbuf.cpu().numpy() == pat).all(), "a refused view was written to"
    # an encode needs nothing to be disjoint
    for name, (v, step) in bad_decode.items():
        assert encode(v, step) == 0, name
    # the bounds themselves — each of the above plus one sample — are accepted
    good = {
        "row_pitch == row": view(pitch=row, istride=(H - 1) * row + row),
        "stacked, image_stride == the window": view(pitch=row + 5, istride=(H - 1) * (row + 5) + row),
        "side by side, image_stride == row": view(pitch=3 * row + row, istride=row),
        "band_stride == the band": view(cols=2, bstride=W * S + win),
    }
    for name, v in good.items():
        assert decode(v) == 0, name
        assert encode(v) == 0, name
    ctx.sync()


# ---- frames as tiles -------------------------------------------------------------------------------------------------------

def test_an_rgba_frame_round_trips_through_tiles(ctx):
    import torch

    from dwt_amd import tiles

    FW, FH, tile = 300, 200, 128
    src = orc.synth(FW, FH, 3, 5, 0)
    pat = V.pattern(FW * FH * 4, False).reshape(FH, FW, 4)
    surface = pat.copy()
    surface[..., :3] = src
    rgba = torch.from_numpy(surface).to(ctx.device)
    coded = tiles.encode_frame(ctx, rgba[..., :3], tile, stepped=True)
    assert len(coded) == 4
    for g, streams, lens, info in coded:
        host, ln = streams.cpu().numpy(), lens.cpu().numpy()
        for i in range(g.cols * g.rows):
            x, y = g.x0 + (i % g.cols) * g.W, g.y0 + (i // g.cols) * g.H
            want, st = orc.encode(src[y:y + g.H, x:x + g.W])
            assert host[i, :ln[i]].tobytes() == want, (g.x0, g.y0, i)
    back = torch.from_numpy(pat).to(ctx.device)
    tiles.decode_frame(ctx, coded, into=back[..., :3], stepped=True)
    got = back.cpu().numpy()
    assert (got[..., :3] == src).all(), "the round trip through tiles is not lossless"
    assert (got[..., 3] == pat[..., 3]).all(), "alpha bytes were written"


# ---- the keyword's default ---------------------------------------------------------------------------------------------------

def test_without_the_keyword_a_stepped_tensor_is_still_refused(ctx):
    import torch

    rgba = torch.zeros((2, 68, 72, 4), dtype=torch.uint8, device=ctx.device)
    streams, info = ctx.encode_view(rgba[..., :3], stepped=True)
    with pytest.raises(ValueError, match="interleaved .* or planar"):
        ctx.encode_view(rgba[..., :3])
    with pytest.raises(ValueError, match="interleaved .* or planar"):
        ctx.decode_view(streams, ctx.stream_lengths(info), rgba[..., :3])
    ctx.sync()


# ---- the stream contract -------------------------------------------------------------------------------------------------

def test_stepped_view_calls_run_on_the_contexts_stream():
    """As tests/test_planar_gpu.py has it for planar views: the frame is filled by a copy queued on the context's own
    stream right before the call, with no synchronisation in between."""
    import torch

    import dwt_amd

    W, H = 132, 100
    L = sgrid(W, H, 3, 4, rows=2)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    c = dwt_amd.Context(0, stream=s.cuda_stream)
    try:
        src = V.pattern(L.samples, False)
        for i, w in enumerate(L.np_windows(src)):
            w[...] = V.picture(W, H, 3, False, i)
        pinned = torch.from_numpy(src).pin_memory()
        rows = [V.oracle_encode(W, H, 3, False, i)[0] for i in range(L.n)]
        with torch.cuda.stream(s):
            tbuf = torch.zeros(L.samples, dtype=torch.uint8, device=dev)
            tbuf.copy_(pinned, non_blocking=True)
            out, info = c.encode_view(L.t_view(tbuf), stepped=True)
            s.synchronize()
            host = out.cpu().numpy()
            for i, I in enumerate(V.infos_of(info)):
                assert host[i, :I.nbytes].tobytes() == rows[i], i
            pat = V.pattern(L.samples, False)
            want = pat.copy()
            for i, w in enumerate(L.np_windows(want)):
                w[...] = V.picture(W, H, 3, False, i)
            pinned_pat = torch.from_numpy(pat).pin_memory()
            lens = c.stream_lengths(info)
            tbuf.copy_(pinned_pat, non_blocking=True)
            c.decode_view(out, lens, L.t_view(tbuf), stepped=True)
            s.synchronize()
            assert (tbuf.cpu().numpy() == want).all()
    finally:
        c.close()
