"""GPU: window lists (dwtx_encode_view_list / dwtx_decode_view_list, include/dwtx.h) — one pointer per picture.

The yardstick is the oracle on each window's copy, exact, as in tests/test_views_gpu.py and tests/test_crop_gpu.py, whose
helpers this file uses: orc for bytes, tests/deep.py for 16-bit samples (maxval 4095), tests/quant.py and tests/floats.py
for float sources and sinks.  A Scatter is a flat patterned buffer with n windows of one shape and one set of strides at
offsets of their own: out of address order, with uneven gaps.  After a decode the WHOLE buffer must equal the expectation —
the picture in each window, the fill everywhere else.  Every layout runs with all pointers on the wide kernels' quad and
with one window moved one sample off it, which sends the whole call through the general conversions."""
import ctypes as C

import numpy as np
import pytest

import deep
import floats
import levels
import orc
import quant
import test_crop_gpu as CR
import test_float_gpu as F
import test_list_cpu as LC
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
M16 = V.M16
N = 5


def up4(v):
    return (v + 3) // 4 * 4


class Scatter:
    """samples: size of the flat buffer; offs: the windows' first samples; shape (H, W, C) and strides (samples) of each."""

    def __init__(self, samples, offs, shape, strides):
        self.samples, self.offs, self.shape, self.strides = samples, list(offs), tuple(shape), tuple(strides)
        self.n = len(self.offs)

    def np_windows(self, buf):
        return [np.lib.stride_tricks.as_strided(buf[o:], self.shape, tuple(s * buf.itemsize for s in self.strides)) for o in self.offs]

    def t_windows(self, tbuf):
        return [tbuf.as_strided(self.shape, self.strides, o) for o in self.offs]

    def on_quad(self):
        return all(o % 4 == 0 for o in self.offs)


GAPS = (12, 40, 4, 28, 20, 8, 36)


def scatter(W, H, Cn, n=N, planar=False, step=0, nudge=None):
    """n windows, each in a slot of its own of one buffer; window i lies in slot (3 * i + 3) % n; pitch, channel stride and
    every slot on the quad; nudge: that window starts one sample later (its gap holds it)."""
    row = W if planar else (W - 1) * (step or Cn) + Cn
    pitch = up4(row) + 8
    cs = H * pitch + 4 if planar else 0
    span = 2 * cs + (H - 1) * pitch + row
    starts, at = [], 8
    for k in range(n):
        starts.append(at)
        at += up4(span) + GAPS[k % len(GAPS)]
    perm = [(3 * i + 3) % n for i in range(n)] if n % 3 else list(range(n))[::-1]
    assert sorted(perm) == list(range(n))
    offs = [starts[p] for p in perm]
    if nudge is not None:
        offs[nudge] += 1
    strides = (pitch, 1, cs) if planar else (pitch, step or Cn, 1)
    return Scatter(at + 8, offs, (H, W, Cn), strides)


# name -> (channels, 16-bit samples, keywords of scatter, keywords of the calls)
LAYOUTS = {
    "gray": (1, False, {}, {}),
    "rgb": (3, False, {}, {}),
    "planar": (3, False, dict(planar=True), {}),
    "rgbx": (3, False, dict(step=4), dict(stepped=True)),
    "bgr": (3, False, {}, dict(order="bgr")),
    "bgrx": (3, False, dict(step=4), dict(stepped=True, order="bgr")),
    "planar-bgr": (3, False, dict(planar=True), dict(order="bgr")),
    "gray16": (1, True, {}, {}),
    "rgb16": (3, True, {}, {}),
    "planar16": (3, True, dict(planar=True), {}),
}
quads = pytest.mark.parametrize("nudge", [None, 2], ids=["quad", "off-quad"])


def in_memory(pic, order):
    return pic[..., ::-1] if order == "bgr" and pic.shape[-1] == 3 else pic


# ---- encode ---------------------------------------------------------------------------------------------------------------

def check_streams(out, info, wants, Cn):
    """wants: (.dwt bytes, oracle stats) per window"""
    infos, host = V.infos_of(info), out.cpu().numpy()
    for i, (want, st) in enumerate(wants):
        I = infos[i]
        assert I.error == 0 and I.nbytes == len(want), i
        assert host[i, :I.nbytes].tobytes() == want, i
        assert list(I.planes)[:Cn] == list(st.planes)[:Cn] and (I.root_bits, I.total_bits) == (st.root_bits, st.total_bits), i


def check_encode(ctx, S, W, H, Cn, is16, pics=None, **call):
    buf = V.pattern(S.samples, is16)
    pics = list(range(S.n)) if pics is None else pics
    for i, w in zip(pics, S.np_windows(buf)):
        w[...] = in_memory(V.picture(W, H, Cn, is16, i), call.get("order"))
    tbuf = V.to_device(ctx, buf)
    out, info = ctx.encode_view_list(S.t_windows(tbuf), **call)
    check_streams(out, info, [V.oracle_encode(W, H, Cn, is16, i) for i in pics], Cn)
    assert (V.to_host(tbuf, is16) == buf).all(), "the source was written to"


# 72x68 wide; 263x135 general; 256x256 16-bit rings and the two-level kernels; 64x64 and 8x8 all tail
ENCODE_CASES = [("gray", 72, 68), ("gray", 256, 256), ("gray", 8, 8), ("rgb", 72, 68), ("rgb", 263, 135), ("planar", 72, 68), ("planar", 64, 64),
                ("rgbx", 72, 68), ("rgbx", 263, 135), ("bgr", 72, 68), ("bgrx", 72, 68), ("planar-bgr", 72, 68), ("gray16", 256, 256),
                ("rgb16", 72, 68), ("planar16", 72, 68)]


@quads
@pytest.mark.parametrize("layout,W,H", ENCODE_CASES, ids=["%s-%dx%d" % c for c in ENCODE_CASES])
def test_encode_list_equals_the_oracle_on_each_window(ctx, layout, W, H, nudge):
    Cn, is16, how, call = LAYOUTS[layout]
    S = scatter(W, H, Cn, nudge=nudge, **how)
    assert S.on_quad() == (nudge is None) and S.offs != sorted(S.offs)
    check_encode(ctx, S, W, H, Cn, is16, **call)


@quads
@pytest.mark.parametrize("kind", floats.KINDS)
@pytest.mark.parametrize("planar", [False, True], ids=["gray", "planar"])
@pytest.mark.parametrize("maxval", [255, M16])
def test_encode_list_of_float_windows(ctx, maxval, planar, kind, nudge):
    W, H, Cn, set_name = 72, 68, 3 if planar else 1, "imagenet_inv"
    scale, bias = quant.SETS[set_name](maxval)
    S = scatter(W, H, Cn, planar=planar, nudge=nudge)
    buf = floats.fill_bits(S.samples, kind)
    for i, w in enumerate(S.np_windows(buf)):
        w[...] = quant.window(W, H, Cn, kind, maxval, set_name, i)[0]
    tf, raw = floats.to_device_floats(ctx.device, buf, kind)
    out, info = ctx.encode_view_list(S.t_windows(tf), maxval=maxval, scale=scale, bias=bias)
    check_streams(out, info, [quant.oracle_encode(W, H, Cn, kind, maxval, set_name, i) for i in range(S.n)], Cn)
    assert (floats.bits_of(raw) == buf).all(), "the source was written to"


def test_encode_list_of_overlapping_and_repeated_windows(ctx):
    """windows that share samples, and one pointer twice: stream i is that of window i's copy"""
    import torch

    W, H, Cn = 72, 68, 3
    frame = orc.synth(2 * W, 2 * H, Cn, 9, 0)
    t = torch.from_numpy(frame).to(ctx.device)
    corners = [(0, 0), (36, 20), (W, H), (36, 20), (8, 1)]
    out, info = ctx.encode_view_list([t[y:y + H, x:x + W] for x, y in corners])
    check_streams(out, info, [orc.encode(np.ascontiguousarray(frame[y:y + H, x:x + W])) for x, y in corners], Cn)


def test_encoder_parts_start_mid_list(ctx):
    """128 windows: the encoder cuts the batch into parts, each of which starts at its own entry of the table"""
    W, H, Cn = 72, 68, 1
    S = scatter(W, H, Cn, n=128)
    check_encode(ctx, S, W, H, Cn, False, pics=[i % N for i in range(S.n)])


# ---- decode ---------------------------------------------------------------------------------------------------------------

def check_decode(ctx, S, W, H, Cn, is16, rows, pixels_max=-1, kind=None, scale=1.0, bias=0.0, size=None, origins=None, order="rgb", **call):
    """rows: one stream per window.  size, origins: the windows are crops of W x H pictures (S holds windows of the crop's size)."""
    buf, want, readable = CR.expectation(S, W, H, Cn, is16, rows, origins or (0, 0), pixels_max, kind, scale, bias, order)
    streams, lens = F.upload(ctx, rows)
    if kind:
        tbuf, raw = floats.to_device_floats(ctx.device, buf, kind)
        more = dict(scale=scale, bias=bias, maxval=M16 if is16 else 255)
    else:
        tbuf = raw = V.to_device(ctx, buf)
        more = dict(maxval=M16 if is16 else None)
    infos = ctx.decode_view_list(streams, lens, S.t_windows(tbuf), size, origins, levels_max=deep.levels_max(W, H, pixels_max), order=order,
                                 **more, **call)
    assert [I.status == 0 for I in infos] == readable
    got = floats.bits_of(raw) if kind else V.to_host(raw, is16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} samples differ, first at {bad[:5]} of {S.samples} (windows at {S.offs}, strides {S.strides})"
    return infos


DECODE_CASES = [("gray", 72, 68), ("gray", 256, 256), ("gray", 8, 8), ("rgb", 72, 68), ("rgb", 263, 135), ("rgb", 64, 64), ("planar", 72, 68),
                ("rgbx", 72, 68), ("bgr", 72, 68), ("planar-bgr", 263, 135), ("gray16", 72, 68), ("rgb16", 256, 256), ("planar16", 72, 68)]


@quads
@pytest.mark.parametrize("layout,W,H", DECODE_CASES, ids=["%s-%dx%d" % c for c in DECODE_CASES])
def test_decode_list_writes_the_windows_and_nothing_else(ctx, layout, W, H, nudge):
    """whole streams, cut() streams, the two mixed, and whole streams under levels_max"""
    Cn, is16, how, call = LAYOUTS[layout]
    S = scatter(W, H, Cn, nudge=nudge, **how)
    for name, rows, pixels_max in V.decode_cases(W, H, Cn, is16, S.n):
        print(name)
        check_decode(ctx, S, W, H, Cn, is16, rows, pixels_max, **call)


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_streams_cut_to_every_level_land_in_the_windows_corners(ctx, Cn):
    W, H = 263, 135   # general whole, wide at 132x68, tail below
    S = scatter(W, H, Cn)
    for name, rows, pixels_max in levels.level_cases(W, H, Cn, False, S.n, names=("stop", "stairs")):
        print(name)
        check_decode(ctx, S, W, H, Cn, False, rows, pixels_max)


@quads
def test_an_unreadable_stream_leaves_its_window_untouched(ctx, nudge):
    W, H, Cn = 72, 68, 3
    S = scatter(W, H, Cn, nudge=nudge)
    rows = CR.whole_rows(W, H, Cn, False, S.n)
    rows[3] = rows[3][:7]
    infos = check_decode(ctx, S, W, H, Cn, False, rows)
    assert [I.status for I in infos] == [0, 0, 0, 1, 0]


SWITCHES = [("decode_parts", 2), ("decode_parts", 4), ("one_stream", 1), ("no_fine16", 1), ("no_square_tiles", 1)]


@pytest.mark.parametrize("name,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
@pytest.mark.parametrize("layout,W,H", [("gray", 256, 256), ("planar", 72, 68), ("rgb", 263, 135)])
def test_decode_list_under_the_switches(ctx, opts, layout, W, H, name, value):
    """decode_parts: the parts of a batch start at entries of the table other than the first"""
    Cn, is16, how, call = LAYOUTS[layout]
    opts.set(name, value)
    S = scatter(W, H, Cn, **how)
    rows = CR.whole_rows(W, H, Cn, is16, S.n)
    check_decode(ctx, S, W, H, Cn, is16, rows, **call)
    rows[1] = V.cut(*V.oracle_encode(W, H, Cn, is16, 1))
    check_decode(ctx, S, W, H, Cn, is16, rows, **call)


def test_decode_list_with_an_offered_index(ctx):
    W, H, Cn = 256, 256, 1
    S = scatter(W, H, Cn)
    rows = CR.whole_rows(W, H, Cn, False, S.n)
    made = ctx.set_index(None, S.n)
    try:
        check_decode(ctx, S, W, H, Cn, False, rows)
        ctx.set_index(made, 0)
        check_decode(ctx, S, W, H, Cn, False, rows)
    finally:
        ctx.set_index()


@quads
@pytest.mark.parametrize("kind", floats.KINDS)
@pytest.mark.parametrize("layout", ["gray", "planar", "rgb", "planar-bgr"])
def test_decode_list_into_float_windows(ctx, layout, kind, nudge):
    W, H = 72, 68
    Cn, is16, how, call = LAYOUTS[layout]
    S = scatter(W, H, Cn, nudge=nudge, **how)
    scale, bias = floats.SETS["imagenet"](255)
    rows = CR.whole_rows(W, H, Cn, False, S.n)
    rows[4] = V.cut(*V.oracle_encode(W, H, Cn, False, 4))
    check_decode(ctx, S, W, H, Cn, False, rows, kind=kind, scale=scale, bias=bias, **call)


def test_decode_list_of_deep_streams_into_float16(ctx):
    W, H = 72, 68
    S = scatter(W, H, 3, planar=True)
    scale, bias = floats.SETS["imagenet"](M16)
    check_decode(ctx, S, W, H, 3, True, CR.whole_rows(W, H, 3, True, S.n), kind="float16", scale=scale, bias=bias)


# ---- crop plus list ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", CR.ROUTES)
@pytest.mark.parametrize("layout", ["gray", "rgb", "planar", "rgbx"])
def test_crops_with_origins_of_their_own_into_listed_windows(ctx, opts, layout, route):
    """whole streams and two that come out at 132x68: one crop partly, one wholly outside the reduced picture"""
    W, H, cw, ch = 263, 135, 30, 20
    Cn, is16, how, call = LAYOUTS[layout]
    T = levels.levels_of(W, H)
    assert levels.sizes(W, H)[T - 1] == (132, 68)
    S = scatter(cw, ch, Cn, **how)
    rows = [levels.stream(W, H, Cn, False, i) for i in range(S.n)]
    for i in (1, 3):
        rows[i] = levels.prefix_for_level(rows[i], W, H, Cn, T - 2)
    origins = [(31, 17), (121, 57), (0, 0), (140, 70), (W - cw, H - ch)]
    opts.set("crop_route", route)
    infos = check_decode(ctx, S, W, H, Cn, False, rows, size=(W, H), origins=origins, **call)
    assert [I.level for I in infos] == [T - 1, T - 2, T - 1, T - 2, T - 1]


def test_crops_into_float_windows_and_a_shared_origin(ctx, opts):
    W, H, cw, ch = 263, 135, 44, 28
    S = scatter(cw, ch, 3, planar=True)
    scale, bias = floats.SETS["imagenet"](255)
    rows = CR.whole_rows(W, H, 3, False, S.n)
    check_decode(ctx, S, W, H, 3, False, rows, kind="float32", scale=scale, bias=bias, size=(W, H), origins=(W - cw, H - ch))
    check_decode(ctx, S, W, H, 3, False, rows, size=(W, H))   # (no origins: every crop at (0, 0))


# ---- separate allocations --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,W,H", [("gray", 72, 68), ("rgb", 263, 135)])
def test_five_tensors_of_their_own(ctx, layout, W, H):
    """each window is a torch.empty of its own with a guard band on either side, which keeps its fill"""
    import torch

    Cn, guard = LAYOUTS[layout][0], 256
    size = W * H * Cn
    fill = V.pattern(2 * guard + size, False)
    rows = CR.whole_rows(W, H, Cn, False, N)
    streams, lens = F.upload(ctx, rows)
    allocs = [torch.empty(2 * guard + size, dtype=torch.uint8, device=ctx.device) for _ in range(N)]
    for a in allocs:
        a.copy_(torch.from_numpy(fill))
    wins = [a[guard:guard + size].view(H, W, Cn) for a in allocs]
    infos = ctx.decode_view_list(streams, lens, wins)
    assert all(I.status == 0 for I in infos)
    for i, a in enumerate(allocs):
        want = fill.copy()
        want[guard:guard + size] = V.picture(W, H, Cn, False, i).reshape(-1)
        assert (a.cpu().numpy() == want).all(), i
    out, info = ctx.encode_view_list(wins[::-1])
    check_streams(out, info, [V.oracle_encode(W, H, Cn, False, i) for i in range(N)][::-1], Cn)


# ---- a list that spells out a grid ------------------------------------------------------------------------------------------

def grid_encode(ctx, v, W, H, n, out, info):
    rc = ctx.lib.dwtx_encode_view(ctx.h, C.byref(v), W, H, n, 0, C.c_void_p(out.data_ptr()), out.shape[1], C.c_void_p(info.data_ptr()))
    assert rc == 0, ctx.lib.dwtx_last_error()


def grid_decode(ctx, v, W, H, n, streams, lens):
    import dwt_amd

    infos = (dwt_amd.DecodeInfo * n)()
    rc = ctx.lib.dwtx_decode_view(ctx.h, C.c_void_p(streams.data_ptr()), streams.shape[1], C.c_void_p(lens.data_ptr()), W, H, n, -1, C.byref(v),
                                  C.cast(infos, C.c_void_p))
    assert rc == 0, ctx.lib.dwtx_last_error()
    return list(infos)


@pytest.mark.parametrize("n", [6, 5], ids=["2x3", "partial-last-band"])
@pytest.mark.parametrize("W,H,Cn", [(72, 68, 3), (263, 135, 1)])
def test_a_list_that_spells_out_a_grid_is_the_grid_call(ctx, W, H, Cn, n):
    import torch

    import dwt_amd

    L = V.grid(W, H, Cn, rows=2, cols=3)
    buf = V.pattern(L.samples, False)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = V.picture(W, H, Cn, False, i)
    src = V.to_device(ctx, buf)
    tv = L.t_view(src)
    wins = [tv[i // 3, i % 3] for i in range(n)]
    v = dwt_amd.View(tv.data_ptr(), 1, Cn, 255, 3, L.strides[2], L.strides[1], L.strides[0], 0)
    stride = ctx.lib.dwtx_encode_bound(W, H, Cn)
    outs = [torch.zeros((n, stride), dtype=torch.uint8, device=ctx.device) for _ in range(2)]
    infos = [torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device) for _ in range(2)]
    grid_encode(ctx, v, W, H, n, outs[0], infos[0])
    ctx.encode_view_list(wins, out=outs[1], info=infos[1])
    ctx.sync()
    assert torch.equal(outs[0], outs[1]) and torch.equal(infos[0], infos[1])
    # decode: whole, cut and unreadable streams into two patterned frames
    rows = CR.whole_rows(W, H, Cn, False, n)
    rows[1] = V.cut(*V.oracle_encode(W, H, Cn, False, 1))
    rows[4] = rows[4][:7]
    streams, lens = F.upload(ctx, rows)
    fill = V.pattern(L.samples, False)
    a, b = V.to_device(ctx, fill), V.to_device(ctx, fill)
    v.dev = L.t_view(a).data_ptr()
    ia = grid_decode(ctx, v, W, H, n, streams, lens)
    tb = L.t_view(b)
    ib = ctx.decode_view_list(streams, lens, [tb[i // 3, i % 3] for i in range(n)])
    assert torch.equal(a, b) and not torch.equal(a, V.to_device(ctx, fill))
    assert [CR.record(I) for I in ia] == [CR.record(I) for I in ib]


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_refused_lists_leave_the_buffer_and_host_info_as_they_were(ctx):
    import dwt_amd

    W, H = LC.W, LC.H
    fill = V.pattern(1 << 16, True)
    tbuf = V.to_device(ctx, fill)   # (2-byte samples: room for every layout in 1- and 2-byte samples)
    assert tbuf.data_ptr() % 16 == 0
    lib = ctx.lib
    for name, ptrs, view, _ in LC.layouts_refused():
        n, Cn, sb = len(ptrs), view.get("channels", 1), view.get("sample_bytes", 1)
        real = [p and p - LC.BASE + tbuf.data_ptr() for p in ptrs]
        assert all(p + 3 * LC.FW * LC.FH * sb < tbuf.data_ptr() + 2 * fill.size for p in real)
        rows = CR.whole_rows(W, H, Cn, sb == 2, n)
        streams, lens = F.upload(ctx, rows)
        v = dwt_amd.View(None, sb, Cn, M16 if sb == 2 else 255, 0, view.get("row_pitch", W * Cn), 0, 0, view.get("channel_stride", 0))
        arr = (C.c_void_p * n)(*[p or None for p in real])
        infos = (dwt_amd.DecodeInfo * n)()
        C.memset(infos, 0x5A, C.sizeof(infos))
        before = bytes(infos)
        rc = lib.dwtx_decode_view_list(ctx.h, C.c_void_p(streams.data_ptr()), streams.shape[1], C.c_void_p(lens.data_ptr()), W, H, n, -1, C.byref(v),
                                       0, 0, None, W, H, None, arr, C.cast(infos, C.c_void_p))
        assert rc == ERR_ARG and lib.dwtx_last_error().strip(), name
        assert dwt_amd.view_list_check(real, W, H, **view)[0] == ERR_ARG, name
        ctx.sync()
        assert bytes(infos) == before, name
        assert (V.to_host(tbuf, True) == fill).all(), name
    # no list at all is refused too: it is not silently the grid call
    v = dwt_amd.View(tbuf.data_ptr(), 1, 1, 255, 0, W, 4096, 0, 0)
    rc = lib.dwtx_decode_view_list(ctx.h, C.c_void_p(streams.data_ptr()), streams.shape[1], C.c_void_p(lens.data_ptr()), W, H, 2, -1, C.byref(v),
                                   0, 0, None, W, H, None, None, C.cast(infos, C.c_void_p))
    assert rc == ERR_ARG and b"list" in lib.dwtx_last_error()
    out = V.to_device(ctx, np.zeros((2, 4096), dtype=np.uint8))
    info = V.to_device(ctx, np.zeros((2, C.sizeof(dwt_amd.StreamInfo)), dtype=np.uint8))
    rc = lib.dwtx_encode_view_list(ctx.h, C.byref(v), 0, 0, None, None, W, H, 2, 0, C.c_void_p(out.data_ptr()), out.shape[1], C.c_void_p(info.data_ptr()))
    assert rc == ERR_ARG and b"list" in lib.dwtx_last_error()
    ctx.sync()
    assert not out.any() and not info.any() and (V.to_host(tbuf, True) == fill).all()


# ---- the host arrays belong to the caller again when the call returns -------------------------------------------------------

def test_the_host_arrays_may_be_overwritten_as_soon_as_the_call_returns(ctx):
    import torch

    import dwt_amd

    W, H, Cn = 72, 68, 1
    S = scatter(W, H, Cn)
    buf = V.pattern(S.samples, False)
    for i, w in enumerate(S.np_windows(buf)):
        w[...] = V.picture(W, H, Cn, False, i)
    tbuf = V.to_device(ctx, buf)
    decoy = torch.zeros(S.samples, dtype=torch.uint8, device=ctx.device)
    pitch = S.strides[0]
    v = dwt_amd.View(None, 1, Cn, 255, 0, pitch, 0, 0, 0)
    arr = (C.c_void_p * S.n)(*[tbuf.data_ptr() + o for o in S.offs])
    stride = ctx.lib.dwtx_encode_bound(W, H, Cn)
    out = torch.zeros((S.n, stride), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros((S.n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
    busy = ctx.synth_pixels(16, 1024, 1024, 1)
    ctx.encode_device(busy)   # (work on the context's stream that the listed call is queued behind)
    rc = ctx.lib.dwtx_encode_view_list(ctx.h, C.byref(v), 0, 0, None, arr, W, H, S.n, 0, C.c_void_p(out.data_ptr()), stride, C.c_void_p(info.data_ptr()))
    for i in range(S.n):
        arr[i] = decoy.data_ptr()
    assert rc == 0, ctx.lib.dwtx_last_error()
    ctx.sync()
    wants = [V.oracle_encode(W, H, Cn, False, i) for i in range(S.n)]
    check_streams(out, info, wants, Cn)
    # the decode: its array and its origins
    cw, ch = 40, 30
    D = scatter(cw, ch, Cn)
    origins = [(3 * i, 2 * i + 1) for i in range(D.n)]
    rows = [w for w, _ in wants]
    fill, want, _ = CR.expectation(D, W, H, Cn, False, rows, origins)
    dbuf = V.to_device(ctx, fill)
    streams, lens = F.upload(ctx, rows)
    v = dwt_amd.View(None, 1, Cn, 255, 0, D.strides[0], 0, 0, 0)
    arr = (C.c_void_p * D.n)(*[dbuf.data_ptr() + o for o in D.offs])
    org = (C.c_int * (2 * D.n))(*[c for o in origins for c in o])
    infos = (dwt_amd.DecodeInfo * D.n)()
    rc = ctx.lib.dwtx_decode_view_list(ctx.h, C.c_void_p(streams.data_ptr()), streams.shape[1], C.c_void_p(lens.data_ptr()), W, H, D.n, -1, C.byref(v),
                                       0, 0, None, cw, ch, org, arr, C.cast(infos, C.c_void_p))
    for i in range(D.n):
        arr[i] = decoy.data_ptr()
        org[2 * i] = org[2 * i + 1] = 0
    assert rc == 0, ctx.lib.dwtx_last_error()
    ctx.sync()
    assert (V.to_host(dbuf, False) == want).all() and not decoy.any()


# ---- history ---------------------------------------------------------------------------------------------------------------

def test_a_plain_call_after_a_listed_call_and_a_list_after_a_list(ctx):
    """on one context of its own: what a call leaves behind (the table's slot, the staging buffer and its event) must not
    show in the next one — every result is the oracle's, which is what a fresh context gives"""
    import dwt_amd

    c = dwt_amd.Context(0)
    try:
        W, H, Cn = 72, 68, 3
        S5, S3 = scatter(W, H, Cn), scatter(W, H, Cn, n=4, nudge=1)
        L = V.grid(W, H, Cn, rows=2, cols=3)
        rows = CR.whole_rows(W, H, Cn, False, 6)
        for _ in range(2):
            check_decode(c, S5, W, H, Cn, False, rows[:5])
            V.check_decode(ctx, L, W, H, Cn, False, rows, view_ctx=c)       # a grid call right after a listed call
            check_decode(c, S3, W, H, Cn, False, rows[2:])                   # another n, other pointers
            check_decode(c, S5, W, H, Cn, False, rows[1:])
            check_encode(c, S5, W, H, Cn, False)
            V.check_encode(c, L, W, H, Cn, False, capacities=(0,))
            check_encode(c, S3, W, H, Cn, False, pics=[3, 1, 0, 2])
            check_encode(c, S5, W, H, Cn, False, pics=[4, 4, 2, 0, 1])
    finally:
        c.close()


# ---- offsets beyond 32 bits -----------------------------------------------------------------------------------------------

@quads
def test_windows_more_than_2_to_the_32_samples_apart(nudge):
    """two windows of one uint8 allocation, 2^32 samples and more apart, the far one first in the list: the place where an
    offset truncated to 32 bits would land holds fill, which must survive.  Compared on the device: the windows and that place."""
    import torch

    import dwt_amd

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    W, H, Cn = 72, 68, 1
    size, FILL = W * H, 0xA5
    near, far = 64, (1 << 32) + (1 << 20) + (0 if nudge is None else 1)
    total = far + size + 4096
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < total * 1.25:
        pytest.skip(f"needs about {total * 1.25 / 2**30:.1f} GiB of free HBM ({free / 2**30:.1f} GiB free)")
    c = dwt_amd.Context(0)
    frame = wins = ghost = None
    try:
        frame = torch.empty(total, dtype=torch.uint8, device=c.device)
        frame.fill_(FILL)
        wins = [frame[far:far + size].view(H, W, Cn), frame[near:near + size].view(H, W, Cn)]
        ghost = frame[near + (far - near) % (1 << 32):][:size]   # where offs[0], cut to 32 bits, would put window 0
        assert ghost.data_ptr() - wins[1].data_ptr() == (wins[0].data_ptr() - wins[1].data_ptr()) % (1 << 32)
        pics = [torch.from_numpy(V.picture(W, H, Cn, False, i)).to(c.device) for i in range(2)]
        rows = CR.whole_rows(W, H, Cn, False, 2)
        streams, lens = F.upload(c, rows)
        infos = c.decode_view_list(streams, lens, wins)
        assert all(I.status == 0 for I in infos)
        assert torch.equal(wins[0], pics[0]) and torch.equal(wins[1], pics[1])
        assert bool((ghost == FILL).all()) and bool((frame[near + size:near + size + 4096] == FILL).all())
        ghost.copy_(pics[1].reshape(-1))   # (an encode that read the truncated place would code the wrong picture)
        out, info = c.encode_view_list(wins)
        check_streams(out, info, [V.oracle_encode(W, H, Cn, False, i) for i in range(2)], Cn)
    finally:
        c.close()
        frame = wins = ghost = None   # (the 4 GiB go back before the next test asks how much is free)
        torch.cuda.empty_cache()
