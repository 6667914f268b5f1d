"""GPU: strided views (dwtx_encode_view / dwtx_decode_view, include/dwtx.h) — windows of a larger frame coded where
they lie — and frames as tile grids (dwt_amd/tiles.py).

The yardstick is the oracle on the cropped copy: orc.encode / orc.decode for bytes, tests/deep.py's pair for 16-bit
samples (maxval 4095).  Every comparison is exact.  A layout is a flat buffer of samples plus an offset, a shape and
strides (in samples): numpy and torch take the same strided view of it, so the expectation of a decode — the oracle's
picture in each window's corner, the prefilled pattern in every other sample of the buffer — is built with numpy alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu

ERR_ARG = -3
M16 = 4095
MY = 3   # rows of frame above and below the windows

# (W, H): 256x256 power-of-two square (16-bit rings, the two-level kernel that writes pixels); 132x100 and 72x68 wide, one
# level at a time; 64x64 and 8x8 the tail; 37x53 and 130x67 the general path
SHAPES = [(256, 256), (132, 100), (72, 68), (64, 64), (8, 8), (37, 53), (130, 67)]
WIDE = [(256, 256), (132, 100), (72, 68)]


# ---- pictures and the oracle ------------------------------------------------------------------------------------

_pics, _enc, _dec = {}, {}, {}


def picture(W, H, Cn, is16, i):
    key = (W, H, Cn, is16, i)
    if key not in _pics:
        _pics[key] = deep.smooth_noise(W, H, Cn, M16, seed=i) if is16 else orc.synth(W, H, Cn, i, 0)
    return _pics[key]


def oracle_encode(W, H, Cn, is16, i, capacity=0):
    key = (W, H, Cn, is16, i, capacity)
    if key not in _enc:
        p = picture(W, H, Cn, is16, i)
        _enc[key] = deep.deep_encode(p, capacity) if is16 else orc.encode(p, capacity)
    return _enc[key]


def oracle_decode(data, W, H, Cn, is16, pixels_max=-1):
    key = (data, W, H, Cn, is16, pixels_max)
    if key not in _dec:
        _dec[key] = deep.deep_decode(data, W, H, Cn, M16, pixels_max) if is16 else orc.decode(data, pixels_max)
    return _dec[key]


def cut(data, st):
    """A prefix that still holds the header and the root image."""
    hdr = (st.meta_bits + st.root_bits + 7) // 8 + 2
    return data[:min(len(data), hdr + (len(data) - hdr) // 3)]


# ---- layouts -------------------------------------------------------------------------------------------------

class Layout:
    """samples: size of the flat buffer; off, shape, strides (samples): the view [n,H,W,C] or [bands,cols,H,W,C]."""

    def __init__(self, samples, off, shape, strides):
        self.samples, self.off, self.shape, self.strides = samples, off, tuple(shape), tuple(strides)
        self.n = int(np.prod(shape[:-3]))

    def np_view(self, buf):
        return np.lib.stride_tricks.as_strided(buf[self.off:], self.shape, tuple(s * buf.itemsize for s in self.strides))

    def np_windows(self, buf):
        v = self.np_view(buf)
        return [v[i] for i in range(self.n)] if v.ndim == 4 else [v[i // self.shape[1], i % self.shape[1]] for i in range(self.n)]

    def t_view(self, tbuf):
        return tbuf.as_strided(self.shape, self.strides, self.off)


def frame_width(W, variant):
    """Columns of a frame that holds four windows side by side, and the windows' left margin.  quad: the windows' first
    samples and the pitch are multiples of 4 samples; off1: the origin is one column off; pitch: the pitch is not."""
    return {"quad": (4 * W + 8, 4), "off1": (4 * W + 12, 5), "pitch": (4 * W + 9, 4)}[variant]


def stack(W, H, Cn, n=3):
    pitch = W * Cn + 5
    slot = H * pitch + 7
    return Layout(3 + n * slot, 3, (n, H, W, Cn), (slot, pitch, Cn, 1))


def band(W, H, Cn, variant="quad"):
    FW, mx = frame_width(W, variant)
    return Layout((H + 2 * MY) * FW * Cn, (MY * FW + mx) * Cn, (4, H, W, Cn), (W * Cn, FW * Cn, Cn, 1))


def grid(W, H, Cn, variant="quad", rows=3, cols=4):
    FW, mx = frame_width(W, variant)
    FW += (cols - 4) * W
    return Layout((rows * H + 2 * MY) * FW * Cn, (MY * FW + mx) * Cn, (rows, cols, H, W, Cn), (H * FW * Cn, W * Cn, FW * Cn, Cn, 1))


LAYOUTS = {"stack": stack, "band": band, "grid": grid}


@functools.lru_cache(maxsize=8)
def _pattern(samples, is16):
    i = np.arange(samples, dtype=np.int64)
    return ((i * 7 + (i >> 9) * 13 + 1) % (4093 if is16 else 251)).astype(np.uint16 if is16 else np.uint8)


def pattern(samples, is16):
    """A buffer's fill (a copy of its own for every caller: the same sizes come again and again)."""
    return _pattern(samples, is16).copy()


def to_device(ctx, buf):
    """numpy samples -> device tensor (16-bit samples travel as int16: the same two bytes, and torch has every operator for them)."""
    import torch

    return torch.from_numpy(buf.view(np.int16) if buf.dtype == np.uint16 else buf).to(ctx.device)


def to_host(t, is16):
    a = t.cpu().numpy()
    return a.view(np.uint16) if is16 else a


def infos_of(info):
    import dwt_amd

    raw = info.cpu().numpy()
    return [dwt_amd.StreamInfo.from_buffer_copy(raw[i].tobytes()) for i in range(raw.shape[0])]


def fields(I):
    return (list(I.planes), I.pmax, I.segments, I.entries, I.tokens, I.order0, I.hdr_bits, I.root_bits, I.meta_bits, I.segments_cut,
            I.total_bits, I.nbytes, I.error)


# ---- encode ----------------------------------------------------------------------------------------------------

def check_encode(ctx, L, W, H, Cn, is16, capacities=(0, 500), first_pic=0):
    buf = pattern(L.samples, is16)   # (whatever lies around the windows must not matter)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = picture(W, H, Cn, is16, first_pic + i)
    tv = L.t_view(to_device(ctx, buf))
    dense = tv.reshape((L.n, H, W, Cn)).contiguous()
    for capacity in capacities:
        out, info = ctx.encode_view(tv, capacity)
        dout, dinfo = (ctx.encode_device16 if is16 else ctx.encode_device)(dense, capacity)
        infos, dinfos = infos_of(info), infos_of(dinfo)
        host, dhost = out.cpu().numpy(), dout.cpu().numpy()
        for i in range(L.n):
            want, st = oracle_encode(W, H, Cn, is16, first_pic + i, capacity)
            I = infos[i]
            assert I.error == 0, (i, capacity)
            assert host[i, :I.nbytes].tobytes() == want, (i, capacity)
            assert list(I.planes)[:Cn] == list(st.planes)[:Cn] and (I.root_bits, I.total_bits) == (st.root_bits, st.total_bits), (i, capacity)
            assert fields(I) == fields(dinfos[i]), (i, capacity)
            assert dhost[i, :I.nbytes].tobytes() == want, (i, capacity)


@pytest.mark.parametrize("layout", ["stack", "band", "grid"])
@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_encode_view_equals_oracle_on_the_crops(ctx, wh, Cn, is16, layout):
    W, H = wh
    check_encode(ctx, LAYOUTS[layout](W, H, Cn), W, H, Cn, is16)


@pytest.mark.parametrize("variant", ["off1", "pitch"])
@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", WIDE, ids=lambda wh: "%dx%d" % wh)
def test_encode_view_off_the_quad_grid(ctx, wh, Cn, is16, variant):
    """Wide shapes whose windows start one column off a quad, or whose pitch is no multiple of 4: the same bytes."""
    W, H = wh
    L = grid(W, H, Cn, variant)
    assert (L.off % 4 != 0) if variant == "off1" else (L.strides[-3] % 4 != 0)
    check_encode(ctx, L, W, H, Cn, is16, capacities=(0,))


# ---- decode ----------------------------------------------------------------------------------------------------

def check_decode(ctx, L, W, H, Cn, is16, rows, pixels_max=-1, view_ctx=None):
    """rows: one stream (bytes) per window.  The whole buffer afterwards: oracle picture in each window's corner, the
    pattern everywhere else."""
    import torch

    n = L.n
    assert len(rows) == n
    buf = pattern(L.samples, is16)
    want = buf.copy()
    for w, data in zip(L.np_windows(want), rows):
        ref = oracle_decode(data, W, H, Cn, is16, pixels_max)
        if ref is not None:
            w[:ref.shape[0], :ref.shape[1]] = ref
    stride = (max(len(r) for r in rows) + 64 + 7) // 8 * 8
    host = np.full((n, stride), 0xA5, dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    streams = torch.from_numpy(host).to(ctx.device)
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)
    tbuf = to_device(ctx, buf)
    infos = (view_ctx or ctx).decode_view(streams, lens, L.t_view(tbuf), maxval=M16 if is16 else None,
                                          levels_max=deep.levels_max(W, H, pixels_max))
    got = to_host(tbuf, is16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} samples differ, first at {bad[:5]} of {L.samples} (view offset {L.off}, strides {L.strides})"
    return infos


def decode_cases(W, H, Cn, is16, n):
    """-> [(name, rows, pixels_max)]: whole streams, all cut, whole and cut mixed (the decoder's non-uniform parts), a level cap."""
    whole, cuts = [], []
    for i in range(n):
        data, st = oracle_encode(W, H, Cn, is16, i)
        whole.append(data)
        cuts.append(cut(data, st))
    g = orc.geometry(W, H)
    cap = g.pixels[max(g.levels - 1, 0)]
    mixed = [cuts[i] if i % 3 == 1 else whole[i] for i in range(n)]
    return [("whole", whole, -1), ("cut", cuts, -1), ("mixed", mixed, -1), ("capped", whole, cap)]


@pytest.mark.parametrize("layout", ["stack", "band", "grid"])
@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_decode_view_writes_the_windows_and_nothing_else(ctx, wh, Cn, is16, layout):
    W, H = wh
    L = LAYOUTS[layout](W, H, Cn)
    for name, rows, pixels_max in decode_cases(W, H, Cn, is16, L.n):
        print(name)
        check_decode(ctx, L, W, H, Cn, is16, rows, pixels_max)


@pytest.mark.parametrize("variant", ["off1", "pitch"])
@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", WIDE, ids=lambda wh: "%dx%d" % wh)
def test_decode_view_off_the_quad_grid(ctx, wh, Cn, is16, variant):
    W, H = wh
    L = grid(W, H, Cn, variant)
    for name, rows, pixels_max in decode_cases(W, H, Cn, is16, L.n)[::2]:   # whole, mixed
        print(name)
        check_decode(ctx, L, W, H, Cn, is16, rows, pixels_max)


# ---- parts: windows that start in the middle of a grid ------------------------------------------------------------------

def test_encoder_parts_start_mid_grid(ctx):
    """128 windows: the encoder cuts the batch into parts, each of which starts at its own window of the 16 x 8 grid."""
    W, H, Cn = 72, 68, 1
    check_encode(ctx, grid(W, H, Cn, "quad", rows=8, cols=16), W, H, Cn, False, capacities=(0,))


@pytest.mark.parametrize("parts", [2, 4])
def test_decoder_parts_start_mid_grid(ctx, opts, parts):
    W, H, Cn = 72, 68, 3
    opts.set("decode_parts", parts)
    L = grid(W, H, Cn, "quad", rows=2, cols=4)
    for name, rows, pixels_max in decode_cases(W, H, Cn, False, L.n)[::2]:
        check_decode(ctx, L, W, H, Cn, False, rows, pixels_max)


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_cols_of_n_or_more_is_one_band(ctx, Cn):
    """A [1, 4, H, W, C] tensor: cols == n, all windows in one band, whatever the band stride says."""
    W, H = 72, 68
    L = grid(W, H, Cn, "quad", rows=1, cols=4)
    check_encode(ctx, L, W, H, Cn, False, capacities=(0,))
    name, rows, pixels_max = decode_cases(W, H, Cn, False, L.n)[2]
    check_decode(ctx, L, W, H, Cn, False, rows, pixels_max)


# ---- frames as tiles ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("FW,FH,Cn,tile,ngroups", [(300, 200, 3, 128, 4), (263, 135, 1, 64, 4)])
def test_frame_round_trip_through_tiles(ctx, FW, FH, Cn, tile, ngroups):
    import torch

    from dwt_amd import tiles

    src = orc.synth(FW, FH, Cn, 5, 0)
    frame = torch.from_numpy(src).to(ctx.device)
    coded = tiles.encode_frame(ctx, frame, tile)
    assert len(coded) == ngroups
    rows = []
    for g, streams, lens, info in coded:
        host, ln = streams.cpu().numpy(), lens.cpu().numpy()
        assert 8 <= g.W <= tile + 7 and 8 <= g.H <= tile + 7
        for i in range(g.cols * g.rows):
            x, y = g.x0 + (i % g.cols) * g.W, g.y0 + (i // g.cols) * g.H
            want, st = orc.encode(src[y:y + g.H, x:x + g.W])
            assert host[i, :ln[i]].tobytes() == want, (g.x0, g.y0, i)
            rows.append((g, i, x, y, want, st))
    back = torch.from_numpy(pattern(FW * FH * Cn, False).reshape(FH, FW, Cn)).to(ctx.device)
    tiles.decode_frame(ctx, coded, into=back)
    assert (back.cpu().numpy() == src).all(), "the round trip through tiles is not lossless"
    # one tile's stream cut short: that tile comes out reduced in its own corner, the rest of it keeps what was there
    g, i, x, y, want, st = rows[len(rows) // 2]
    hdr = (st.meta_bits + st.root_bits + 7) // 8
    for keep in (hdr + 4, hdr + 16, hdr + 64, hdr + 256):   # the shortest of these prefixes the oracle reads
        short = want[:keep]
        ref = orc.decode(short)
        if ref is not None:
            break
    assert ref is not None and ref.shape[0] < g.H and ref.shape[1] < g.W
    lens2 = [c[2].clone() for c in coded]
    k = [c[0] is g for c in coded].index(True)
    lens2[k][i] = len(short)
    pat = pattern(FW * FH * Cn, False).reshape(FH, FW, Cn)
    back = torch.from_numpy(pat).to(ctx.device)
    tiles.decode_frame(ctx, [(c[0], c[1], l) for c, l in zip(coded, lens2)], into=back)
    expect = src.copy()
    expect[y:y + g.H, x:x + g.W] = pat[y:y + g.H, x:x + g.W]
    expect[y:y + ref.shape[0], x:x + ref.shape[1]] = ref
    assert (back.cpu().numpy() == expect).all()


# ---- argument rules ---------------------------------------------------------------------------------------------------

def test_bad_views_are_refused_and_nothing_is_written(ctx):
    import torch

    import dwt_amd

    W, H, Cn, n = 72, 68, 1, 4
    FW = 4 * W + 8
    pat = pattern((H * 2 + 8) * FW + 64, False)
    tbuf = to_device(ctx, pat)
    tbuf16 = to_device(ctx, pattern(pat.size, True))
    data, _ = oracle_encode(W, H, Cn, False, 0)
    stride = (len(data) + 64 + 7) // 8 * 8
    host = np.zeros((n, stride), dtype=np.uint8)
    host[:, :len(data)] = np.frombuffer(data, dtype=np.uint8)
    streams = torch.from_numpy(host).to(ctx.device)
    lens = torch.full((n,), len(data), dtype=torch.int64, device=ctx.device)
    out = torch.zeros((n, 8192), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()
    p8, p16 = tbuf.data_ptr(), tbuf16.data_ptr()
    row, win = W * Cn, (H - 1) * FW + W * Cn

    def view(dev=p8, sb=1, ch=Cn, maxval=255, cols=0, pitch=FW, istride=W * Cn, bstride=0):
        return dwt_amd.View(dev, sb, ch, maxval, cols, pitch, istride, bstride)

    def decode(v, count=n):
        return ctx.lib.dwtx_decode_view(ctx.h, streams.data_ptr(), stride, lens.data_ptr(), W, H, count, -1, C.byref(v),
                                        C.cast(infos, C.c_void_p))

    def encode(v):
        return ctx.lib.dwtx_encode_view(ctx.h, C.byref(v), W, H, n, 0, out.data_ptr(), out.shape[1], info.data_ptr())

    bad_both = {
        "row_pitch below a row": view(pitch=row - 1),
        "unaligned 16-bit samples": view(dev=p16 + 1, sb=2, maxval=M16),
        "sample_bytes": view(sb=4),
        "channels": view(ch=2),
    }
    bad_decode = {
        "side by side, overlapping columns": view(istride=row - 1),
        "side by side, pitch too short for the band": view(pitch=3 * row + row - 1, istride=row),
        "stacked, slots overlap": view(pitch=row, istride=(H - 1) * row + row - 1),
        "bands overlap": view(cols=2, bstride=row + win - 1),
        "maxval with bytes": view(maxval=254),
        "maxval beyond 16 bits": view(dev=p16, sb=2, maxval=65536),
    }
    for name, v in {**bad_both, **bad_decode}.items():
        assert decode(v) == ERR_ARG, name
        assert ctx.lib.dwtx_last_error(), name
    for name, v in bad_both.items():
        assert encode(v) == ERR_ARG, name
    ctx.sync()
    assert (tbuf.cpu().numpy() == pat).all() and (to_host(tbuf16, True) == pattern(pat.size, True)).all()
    # the bounds themselves are fine: one sample more, and overlapping sources of an encode
    for name in ("side by side, pitch too short for the band", "bands overlap"):
        v = bad_decode[name]
        if name.startswith("side"):
            v.row_pitch += 1
        else:
            v.band_stride += 1
        assert decode(v) == 0, name
    assert encode(bad_decode["side by side, overlapping columns"]) == 0
    ctx.sync()


# ---- the stream contract --------------------------------------------------------------------------------------------------

def test_view_calls_run_on_the_contexts_stream():
    """A context on a torch stream of its own: the frame is filled by a copy queued on that stream right before the call,
    with no synchronisation in between."""
    import torch

    import dwt_amd

    W, H, Cn = 132, 100, 3
    L = grid(W, H, Cn, "quad", rows=2, cols=4)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    c = dwt_amd.Context(0, stream=s.cuda_stream)
    try:
        src = pattern(L.samples, False)
        for i, w in enumerate(L.np_windows(src)):
            w[...] = picture(W, H, Cn, False, i)
        pinned = torch.from_numpy(src).pin_memory()
        rows = [oracle_encode(W, H, Cn, False, i)[0] for i in range(L.n)]
        with torch.cuda.stream(s):
            tbuf = torch.zeros(L.samples, dtype=torch.uint8, device=dev)
            tbuf.copy_(pinned, non_blocking=True)
            out, info = c.encode_view(L.t_view(tbuf))
            s.synchronize()
            host = out.cpu().numpy()
            for i, I in enumerate(infos_of(info)):
                assert host[i, :I.nbytes].tobytes() == rows[i], i
            # decode: the pattern lands on the stream, then the windows
            pat = pattern(L.samples, False)
            want = pat.copy()
            for i, w in enumerate(L.np_windows(want)):
                w[...] = picture(W, H, Cn, False, i)
            pinned_pat = torch.from_numpy(pat).pin_memory()
            lens = c.stream_lengths(info)
            tbuf.copy_(pinned_pat, non_blocking=True)
            c.decode_view(out, lens, L.t_view(tbuf))
            s.synchronize()
            assert (tbuf.cpu().numpy() == want).all()
    finally:
        c.close()
