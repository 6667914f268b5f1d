"""GPU: planar (channel-first) RGB in strided views — dwtx_view.channel_stride (include/dwtx.h): NCHW stacks, the tile
grid of a CHW frame and CNHW batches coded where they lie.

The yardstick is that of tests/test_views_gpu.py, whose helpers this file uses: the oracle on the interleaved crop, exact,
and for a decode every sample of a pattern-prefilled buffer.  A planar layout is a Layout like any other — shape
[n,H,W,3] or [bands,cols,H,W,3] with column stride 1 and the channel stride last — so numpy's and torch's strided views
of the flat buffer build the expectations."""
import ctypes as C

import numpy as np
import pytest

import orc
import test_views_gpu as V
from test_views_gpu import Layout, MY

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG


def up4(v):
    return (v + 3) // 4 * 4


# ---- layouts: all C = 3.  variant "quad": origin, pitch and channel stride multiples of 4 samples (what the wide kernels
# ask); "off3": the origin is not; "pitch5": the pitch is not; "csodd": the channel stride is not — one at a time

def nchw(W, H, variant="quad", n=3):
    """Planes inside the window: three padded pictures, each its three padded planes."""
    off = 3 if variant == "off3" else 4
    pitch = W + (5 if variant == "pitch5" else 8)
    cs = up4(H * pitch + 12) + (1 if variant == "csodd" else 0)
    slot = up4(3 * cs + 4)
    return Layout(off + n * slot, off, (n, H, W, 3), (slot, pitch, 1, cs))


def chw_grid(W, H, variant="quad", rows=2, cols=4):
    """A rows x cols tile grid of one planar frame with MY margin rows and a left margin; the channel stride is the padded
    frame plane."""
    FW = cols * W + (9 if variant == "pitch5" else 8)
    mx = 3 if variant == "off3" else 4
    FH = rows * H + 2 * MY
    cs = up4(FH * FW) + (1 if variant == "csodd" else 0)
    return Layout(2 * cs + FH * FW, MY * FW + mx, (rows, cols, H, W, 3), (H * FW, W, FW, 1, cs))


def cnhw(W, H, variant="quad", n=3):
    """Stacked windows, the channel planes of the whole batch apart."""
    off = 3 if variant == "off3" else 4
    pitch = W + (5 if variant == "pitch5" else 8)
    slot = up4(H * pitch + 4)
    cs = n * slot + 8 + (1 if variant == "csodd" else 0)
    return Layout(off + 2 * cs + n * slot, off, (n, H, W, 3), (slot, pitch, 1, cs))


LAYOUTS = {"nchw": nchw, "chw_grid": chw_grid, "cnhw": cnhw}
depths = pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
shapes = pytest.mark.parametrize("wh", V.SHAPES, ids=lambda wh: "%dx%d" % wh)
wide_shapes = pytest.mark.parametrize("wh", V.WIDE, ids=lambda wh: "%dx%d" % wh)


def test_the_quad_layouts_are_on_the_quad_grid():
    for make in LAYOUTS.values():
        L = make(72, 68)
        assert L.off % 4 == 0 and all(s % 4 == 0 for s in L.strides[:-3] + L.strides[-3:-2] + L.strides[-1:]), L.strides
        assert L.strides[-2] == 1


# ---- encode, decode ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(LAYOUTS))
@depths
@shapes
def test_planar_encode_equals_oracle_on_the_interleaved_crops(ctx, wh, is16, layout):
    W, H = wh
    V.check_encode(ctx, LAYOUTS[layout](W, H), W, H, 3, is16)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@depths
@shapes
def test_planar_decode_writes_the_windows_planes_and_nothing_else(ctx, wh, is16, layout):
    W, H = wh
    L = LAYOUTS[layout](W, H)
    for name, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n):
        print(name)
        V.check_decode(ctx, L, W, H, 3, is16, rows, pixels_max)


@pytest.mark.parametrize("variant", ["off3", "pitch5", "csodd"])
@depths
@wide_shapes
def test_planar_off_the_quad_grid(ctx, wh, is16, variant):
    """Wide shapes whose origin, pitch or channel stride is off the quad grid take the general path: the same bytes."""
    W, H = wh
    L = nchw(W, H, variant)
    assert {"off3": L.off, "pitch5": L.strides[1], "csodd": L.strides[3]}[variant] % 4 != 0
    assert sum(v % 4 != 0 for v in (L.off, L.strides[0], L.strides[1], L.strides[3])) == 1
    V.check_encode(ctx, L, W, H, 3, is16, capacities=(0,))
    for name, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n)[::2]:   # whole, mixed
        print(name)
        V.check_decode(ctx, L, W, H, 3, is16, rows, pixels_max)


SWITCHES = [("no_fused_levels", 1), ("no_fine16", 1), ("no_pixels16", 1), ("no_square_tiles", 1), ("lift_rows", 4), ("lift_rows", 64)]
# (no_pixels16 is about deep pixels only)
SWITCH_CASES = [pytest.param(name, value, is16, id="%s=%d-%s" % (name, value, "u16" if is16 else "u8"))
                for name, value in SWITCHES for is16 in (False, True) if is16 or name != "no_pixels16"]


@pytest.mark.parametrize("name,value,is16", SWITCH_CASES)
@wide_shapes
def test_planar_under_the_switches(ctx, opts, wh, name, value, is16):
    """The code paths the diagnostic switches choose between agree on planar pixels too."""
    W, H = wh
    opts.set(name, value)
    L = nchw(W, H)
    V.check_encode(ctx, L, W, H, 3, is16, capacities=(0,))
    for case, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n)[::2]:
        print(case)
        V.check_decode(ctx, L, W, H, 3, is16, rows, pixels_max)


# 128 wide: the histograms ride along on the finest level; 260: one lane into a second strip; heights 131 and 514: a last row
# pair without its odd row, and under lift_rows 16 / 64 strips of a single row pair (the batches of the 8-bit planar
# kernel are one row pair, the others' two: their last batch ends differently)
STRIP_EDGES = [(128, 130), (260, 131), (68, 514)]


@pytest.mark.parametrize("rows", [16, 64])
@depths
@pytest.mark.parametrize("wh", STRIP_EDGES, ids=lambda wh: "%dx%d" % wh)
def test_planar_rows_per_wave_at_the_strip_edges(ctx, opts, wh, is16, rows):
    W, H = wh
    opts.set("lift_rows", rows)
    V.check_encode(ctx, nchw(W, H), W, H, 3, is16, capacities=(0,))


# ---- parts -------------------------------------------------------------------------------------------------------------

def test_planar_encoder_parts_start_mid_grid(ctx):
    """128 windows: the encoder's parts each start at a window of their own of the 16 x 8 planar grid."""
    W, H = 72, 68
    V.check_encode(ctx, chw_grid(W, H, rows=8, cols=16), W, H, 3, False, capacities=(0,))


@pytest.mark.parametrize("parts", [2, 4])
def test_planar_decoder_parts_start_mid_grid(ctx, opts, parts):
    W, H = 72, 68
    opts.set("decode_parts", parts)
    L = chw_grid(W, H)
    for name, rows, pixels_max in V.decode_cases(W, H, 3, False, L.n)[::2]:
        V.check_decode(ctx, L, W, H, 3, False, rows, pixels_max)


# ---- torch's own layouts through the public API ------------------------------------------------------------------------

def test_an_nchw_tensor_is_a_view_as_it_is(ctx):
    import torch

    W, H, n = 72, 68, 4
    pics = [V.picture(W, H, 3, False, i) for i in range(n)]
    t = torch.from_numpy(np.stack(pics).transpose(0, 3, 1, 2).copy()).to(ctx.device)
    assert t.shape == (n, 3, H, W) and t.is_contiguous()
    nhwc = t.permute(0, 2, 3, 1)
    out, info = ctx.encode_view(nhwc)
    dout, dinfo = ctx.encode_device(nhwc.contiguous())
    host, dhost = out.cpu().numpy(), dout.cpu().numpy()
    rows = []
    for i, (I, D) in enumerate(zip(V.infos_of(info), V.infos_of(dinfo))):
        want, st = V.oracle_encode(W, H, 3, False, i)
        assert V.fields(I) == V.fields(D) and I.error == 0, i
        assert host[i, :I.nbytes].tobytes() == want and dhost[i, :D.nbytes].tobytes() == want, i
        rows.append(V.cut(want, st) if i == 2 else want)
    pat = V.pattern(n * 3 * H * W, False).reshape(n, 3, H, W)
    want = pat.copy()
    for i, data in enumerate(rows):
        ref = V.oracle_decode(data, W, H, 3, False)
        want[i, :, :ref.shape[0], :ref.shape[1]] = ref.transpose(2, 0, 1)
    back = torch.from_numpy(pat).to(ctx.device)
    stride = (max(len(r) for r in rows) + 64 + 7) // 8 * 8
    sh = np.zeros((n, stride), dtype=np.uint8)
    for i, r in enumerate(rows):
        sh[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)
    ctx.decode_view(torch.from_numpy(sh).to(ctx.device), lens, back.permute(0, 2, 3, 1))
    assert (back.cpu().numpy() == want).all()


def test_a_chw_frame_round_trips_through_tiles(ctx):
    """tests/test_views_gpu.py's frame test on a planar frame: [3,200,300] permuted to [200,300,3], no copy."""
    import torch

    from dwt_amd import tiles

    FW, FH, tile = 300, 200, 128
    src = orc.synth(FW, FH, 3, 5, 0)
    chw = torch.from_numpy(src.transpose(2, 0, 1).copy()).to(ctx.device)
    assert chw.shape == (3, FH, FW) and chw.is_contiguous()
    coded = tiles.encode_frame(ctx, chw.permute(1, 2, 0), tile)
    assert len(coded) == 4
    rows = []
    for g, streams, lens, info in coded:
        host, ln = streams.cpu().numpy(), lens.cpu().numpy()
        for i in range(g.cols * g.rows):
            x, y = g.x0 + (i % g.cols) * g.W, g.y0 + (i // g.cols) * g.H
            want, st = orc.encode(src[y:y + g.H, x:x + g.W])
            assert host[i, :ln[i]].tobytes() == want, (g.x0, g.y0, i)
            rows.append((g, i, x, y, want, st))
    pat = V.pattern(FW * FH * 3, False).reshape(3, FH, FW)
    back = torch.from_numpy(pat).to(ctx.device)
    tiles.decode_frame(ctx, coded, into=back.permute(1, 2, 0))
    assert (back.cpu().numpy() == src.transpose(2, 0, 1)).all(), "the round trip through planar tiles is not lossless"
    # one tile's stream cut short: reduced in its own corner of each plane, the rest of the tile keeps what was there
    g, i, x, y, want, st = rows[len(rows) // 2]
    hdr = (st.meta_bits + st.root_bits + 7) // 8
    for keep in (hdr + 4, hdr + 16, hdr + 64, hdr + 256):
        short = want[:keep]
        ref = orc.decode(short)
        if ref is not None:
            break
    assert ref is not None and ref.shape[0] < g.H and ref.shape[1] < g.W
    lens2 = [c[2].clone() for c in coded]
    k = [c[0] is g for c in coded].index(True)
    lens2[k][i] = len(short)
    back = torch.from_numpy(pat).to(ctx.device)
    tiles.decode_frame(ctx, [(c[0], c[1], l) for c, l in zip(coded, lens2)], into=back.permute(1, 2, 0))
    expect = src.transpose(2, 0, 1).copy()
    expect[:, y:y + g.H, x:x + g.W] = pat[:, y:y + g.H, x:x + g.W]
    expect[:, y:y + ref.shape[0], x:x + ref.shape[1]] = ref.transpose(2, 0, 1)
    assert (back.cpu().numpy() == expect).all()


def test_other_strides_are_still_refused(ctx):
    import torch

    t = torch.zeros((2, 68, 72, 6), dtype=torch.uint8, device=ctx.device)
    for bad in (t[..., ::2], t[:, :, ::2, :3], t[..., :2]):   # channel stride 2, column stride 12, two channels
        with pytest.raises(ValueError, match="interleaved .* or planar"):
            ctx.encode_view(bad)


# ---- argument rules, through ctypes -------------------------------------------------------------------------------------

def test_bad_planar_views_are_refused_and_nothing_is_written(ctx):
    import torch

    import dwt_amd

    W, H, n = 72, 68, 4
    pitch = W + 8
    pw = (H - 1) * pitch + W          # a plane of a window
    win = 3 * pw                      # first form, tight: channel_stride = pw, so win = 2 * pw + pw
    span = 3 * pw + pw                # second form: four stacked windows of one channel, image_stride = pw
    pat = V.pattern(16 * pw + 64, False)
    tbuf = V.to_device(ctx, pat)
    data, _ = V.oracle_encode(W, H, 3, False, 0)
    gray, _ = V.oracle_encode(W, H, 1, False, 0)
    stride = (max(len(data), len(gray)) + 64 + 7) // 8 * 8

    def rows_of(d):
        host = np.zeros((n, stride), dtype=np.uint8)
        host[:, :len(d)] = np.frombuffer(d, dtype=np.uint8)
        return torch.from_numpy(host).to(ctx.device), torch.full((n,), len(d), dtype=torch.int64, device=ctx.device)

    streams, lens = rows_of(data)
    out = torch.zeros((n, 3 * 8192), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()

    def view(dev=None, ch=3, cols=0, pitch=pitch, istride=win, bstride=0, cs=pw):
        return dwt_amd.View(tbuf.data_ptr() if dev is None else dev, 1, ch, 255, cols, pitch, istride, bstride, cs)

    def decode(v, s=streams, l=lens):
        return ctx.lib.dwtx_decode_view(ctx.h, s.data_ptr(), stride, l.data_ptr(), W, H, n, -1, C.byref(v), C.cast(infos, C.c_void_p))

    def encode(v, o=out):
        return ctx.lib.dwtx_encode_view(ctx.h, C.byref(v), W, H, n, 0, o.data_ptr(), o.shape[1], info.data_ptr())

    band = win + win                  # two windows of a band, first form
    bad = {
        "row_pitch below a plane's row": view(pitch=W - 1),
        "planes of a window overlap (first form)": view(cs=pw - 1),
        "windows overlap (first form)": view(istride=win - 1),
        "bands overlap": view(cols=2, bstride=band - 1),
        "planes of the whole view overlap (second form)": view(istride=pw, cs=span - 1),
    }
    for name, v in bad.items():
        assert decode(v) == ERR_ARG, name
        assert ctx.lib.dwtx_last_error(), name
    assert encode(bad["row_pitch below a plane's row"]) == ERR_ARG and ctx.lib.dwtx_last_error()
    ctx.sync()
    assert (tbuf.cpu().numpy() == pat).all(), "a refused view was written to"
    # an encode needs nothing to be disjoint
    for name in list(bad)[1:]:
        assert encode(bad[name]) == 0, name
    # the bounds themselves — each of the above plus one sample — are fine
    good = {
        "row_pitch == W": view(pitch=W, istride=3 * H * W, cs=H * W),
        "channel_stride == pw, image_stride == win": view(),
        "band_stride == the band": view(cols=2, bstride=band),
        "channel_stride == one channel of the whole view": view(istride=pw, cs=span),
    }
    for name, v in good.items():
        assert decode(v) == 0, name
    ctx.sync()
    # channels == 1: the field is ignored
    gs, gl = rows_of(gray)
    a, b = V.to_device(ctx, pat), V.to_device(ctx, pat)
    for buf, cs in ((a, 0), (b, 12345)):
        v = dwt_amd.View(buf.data_ptr(), 1, 1, 255, 0, pitch, pw, 0, cs)
        assert decode(v, gs, gl) == 0
    ctx.sync()
    assert (a.cpu().numpy() == b.cpu().numpy()).all() and (a.cpu().numpy() != pat).any()
    outs = []
    for cs in (0, 12345):
        o = torch.zeros((n, 8192), dtype=torch.uint8, device=ctx.device)
        assert encode(dwt_amd.View(a.data_ptr(), 1, 1, 255, 0, pitch, pw, 0, cs), o) == 0
        ctx.sync()
        outs.append(o.cpu().numpy())
    assert (outs[0] == outs[1]).all() and outs[0][0, :len(gray)].tobytes() == gray


# ---- interleaved pixels are what they were --------------------------------------------------------------------------------

def test_channel_stride_zero_is_the_interleaved_path(ctx):
    W, H = 132, 100
    L = V.grid(W, H, 3)
    V.check_encode(ctx, L, W, H, 3, False, capacities=(0,))
    name, rows, pixels_max = V.decode_cases(W, H, 3, False, L.n)[2]
    V.check_decode(ctx, L, W, H, 3, False, rows, pixels_max)


# ---- the stream contract -------------------------------------------------------------------------------------------------

def test_planar_view_calls_run_on_the_contexts_stream():
    """As tests/test_views_gpu.py has it for interleaved views: the frame is filled by a copy queued on the context's own
    stream right before the call, with no synchronisation in between."""
    import torch

    import dwt_amd

    W, H = 132, 100
    L = chw_grid(W, H)
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
            out, info = c.encode_view(L.t_view(tbuf))
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
            c.decode_view(out, lens, L.t_view(tbuf))
            s.synchronize()
            assert (tbuf.cpu().numpy() == want).all()
    finally:
        c.close()
