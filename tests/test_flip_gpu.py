"""GPU: flips in views (dwtx_encode_view_flip / dwtx_decode_view_flip, include/dwtx.h) — bottom-up surfaces and mirrored
pictures coded where they lie.

The yardstick is the oracle on the UPRIGHT pictures, exact, as in tests/test_views_gpu.py, tests/test_list_gpu.py and
tests/test_crop_gpu.py, whose helpers this file uses; what a window holds in memory follows from a picture with
tests/flip.py (in_memory, place), which tests/test_flip_cpu.py holds against hand-written cases.  A source is compared
after every encode, and after every decode the WHOLE buffer: the picture in each window — a reduced one in the corner where
its pixel (0, 0) lies — and the fill everywhere else.  Every layout runs as a grid (no list: the view's own windows) and as
a scattered list, with all windows on the wide kernels' quad and off it, under one mask for all windows (1, 2, 3) and under
the per-picture lists [0, 1, 2, 3, 1] and [0, 2, 2, 0, 2]."""
import ctypes as C
import random

import numpy as np
import pytest

import deep
import flip
import floats
import levels
import orc
import quant
import test_crop_gpu as CR
import test_encode_index_gpu as EI
import test_float_gpu as F
import test_list_gpu as LG
import test_step_gpu as S
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
M16 = V.M16
N = 5
BOTTOM_UP = [0, 2, 2, 0, 2]   # upright and bottom-up windows in one call: what the wide forward kernels take per window
FLAGSETS = [1, 2, 3, flip.MIXED, BOTTOM_UP]
# what an on-quad window of each shape reaches, flipped as unflipped (profiles/flip_kernel_calls.txt has the names): 72x68 the wide
# kernels; 256x256 16-bit rings and the pixel-writing pair kernels; 520x264 wide, reduced to 260x132 wide and 130x66 general;
# 263x135 general, reduced 132x68 wide inside a window whose width is no multiple of 4 (a mirrored one: general); 64x64 and 8x8 all tail
SHAPES = [(72, 68), (256, 256), (520, 264), (263, 135), (64, 64), (8, 8)]


def flags_of(fs, n=N):
    return [fs] * n if isinstance(fs, int) else list(fs)


def gridded(W, H, Cn, n=N, planar=False, step=0, nudge=None):
    """the windows of LG.scatter as a stack, which a view describes: the grid side of every layout; nudge: the view starts one
    sample off the quad"""
    row = W if planar else (W - 1) * (step or Cn) + Cn
    pitch = LG.up4(row) + 8
    cs = H * pitch + 4 if planar else 0
    slot = LG.up4(2 * cs + (H - 1) * pitch + row) + 12
    off = 8 + (0 if nudge is None else 1)
    return V.Layout(off + n * slot + 8, off, (n, H, W, Cn), (slot, pitch, 1, cs) if planar else (slot, pitch, step or Cn, 1))


def windows_of(how, W, H, Cn, nudge, n=N, **kw):
    return gridded(W, H, Cn, n=n, nudge=nudge, **kw) if how == "grid" else LG.scatter(W, H, Cn, n=n, nudge=nudge, **kw)


def shape_for(rng, k):
    return SHAPES[(rng.randrange(len(SHAPES)) + k) % len(SHAPES)]


hows = pytest.mark.parametrize("how", ["grid", "list"])
quads = LG.quads


# ---- 1. encode -----------------------------------------------------------------------------------------------------------------

def encode(ctx, L, tbuf, flags, capacity=0, **call):
    if isinstance(L, LG.Scatter):
        return ctx.encode_view_list(L.t_windows(tbuf), capacity=capacity, flip=flags, **call)
    return ctx.encode_view(L.t_view(tbuf), capacity, flip=flags, **call)


def check_encode(ctx, L, W, H, Cn, is16, fs, capacity=0, **call):
    flags = flags_of(fs, L.n)
    buf = V.pattern(L.samples, is16)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = flip.in_memory(LG.in_memory(V.picture(W, H, Cn, is16, i), call.get("order")), flags[i])
    tbuf = V.to_device(ctx, buf)
    out, info = encode(ctx, L, tbuf, fs, capacity, **call)
    LG.check_streams(out, info, [V.oracle_encode(W, H, Cn, is16, i, capacity) for i in range(L.n)], Cn)
    assert (V.to_host(tbuf, is16) == buf).all(), "the source was written to"
    return out, info


@quads
@hows
@pytest.mark.parametrize("layout", list(LG.LAYOUTS))
def test_flipped_encode_equals_the_oracle_on_the_upright_pictures(ctx, layout, how, nudge):
    """every layout x flags x (grid | list) x (quad | off); the shape of each by a seeded choice that walks through all six"""
    Cn, is16, kw, call = LG.LAYOUTS[layout]
    rng = random.Random(f"enc {layout} {how} {nudge}")
    for k, fs in enumerate(FLAGSETS):
        W, H = shape_for(rng, k)
        print(fs, W, H)
        check_encode(ctx, windows_of(how, W, H, Cn, nudge, **kw), W, H, Cn, is16, fs, **call)


@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_flipped_encode_of_every_shape(ctx, wh):
    """the sweep above samples shapes: here each of them under the mixed flags, gray on a grid and RGB as a list"""
    W, H = wh
    check_encode(ctx, windows_of("grid", W, H, 1, None), W, H, 1, False, flip.MIXED)
    check_encode(ctx, windows_of("list", W, H, 3, None), W, H, 3, False, flip.MIXED)


@hows
@pytest.mark.parametrize("layout,W,H", [("gray", 256, 256), ("rgb", 72, 68), ("planar", 263, 135), ("rgbx", 72, 68), ("gray16", 72, 68)])
def test_flipped_encode_under_a_capacity(ctx, layout, W, H, how):
    Cn, is16, kw, call = LG.LAYOUTS[layout]
    check_encode(ctx, windows_of(how, W, H, Cn, None, **kw), W, H, Cn, is16, flip.MIXED, capacity=500, **call)


@quads
@hows
@pytest.mark.parametrize("kind", floats.KINDS)
@pytest.mark.parametrize("planar", [False, True], ids=["gray", "planar"])
@pytest.mark.parametrize("maxval", [255, M16])
def test_flipped_encode_of_float_windows(ctx, maxval, planar, kind, how, nudge):
    W, H, Cn, set_name = 72, 68, 3 if planar else 1, "imagenet_inv"
    scale, bias = quant.SETS[set_name](maxval)
    L = windows_of(how, W, H, Cn, nudge, planar=planar)
    wants = [quant.oracle_encode(W, H, Cn, kind, maxval, set_name, i) for i in range(L.n)]
    for fs in FLAGSETS:
        flags = flags_of(fs)
        buf = floats.fill_bits(L.samples, kind)
        for i, w in enumerate(L.np_windows(buf)):
            w[...] = flip.in_memory(quant.window(W, H, Cn, kind, maxval, set_name, i)[0], flags[i])
        tf, raw = floats.to_device_floats(ctx.device, buf, kind)
        if how == "list":
            out, info = ctx.encode_view_list(L.t_windows(tf), maxval=maxval, scale=scale, bias=bias, flip=fs)
        else:
            out, info = ctx.encode_view_float(L.t_view(tf), maxval=maxval, scale=scale, bias=bias, flip=fs)
        LG.check_streams(out, info, wants, Cn)
        assert (floats.bits_of(raw) == buf).all(), "the source was written to"


@hows
def test_the_encode_index_of_a_flipped_encode_is_that_of_the_upright_pictures(ctx, how):
    W, H, Cn = 256, 256, 3
    L = windows_of(how, W, H, Cn, None)
    pics = [V.picture(W, H, Cn, False, i) for i in range(L.n)]
    dev_index = ctx.set_encode_index(L.n, device=True)
    try:
        out, info = check_encode(ctx, L, W, H, Cn, False, flip.MIXED)
        got = EI._rows(ctx, dev_index)
        ctx.encode_device(V.to_device(ctx, np.stack(pics)))
        want = EI._rows(ctx, dev_index)
    finally:
        ctx.set_encode_index()
    EI._assert_equal(got, want, "flipped encode")


@pytest.mark.parametrize("masks", [(0, 1, 2, 3), (0, 2)], ids=["any", "bottom-up"])
def test_flipped_encoder_parts_start_mid_list(ctx, masks):
    """128 windows: the encoder's parts start at their own entries of the table, flags and all — through the general conversion
    (a mirrored window among them) and through the wide forward kernels (upright and bottom-up windows only)"""
    W, H, Cn = 72, 68, 1
    L = LG.scatter(W, H, Cn, n=128)
    flags = [masks[(i * 7 + i // 5) % len(masks)] for i in range(L.n)]
    buf = V.pattern(L.samples, False)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = flip.in_memory(V.picture(W, H, Cn, False, i % N), flags[i])
    out, info = ctx.encode_view_list(L.t_windows(V.to_device(ctx, buf)), flip=flags)
    LG.check_streams(out, info, [V.oracle_encode(W, H, Cn, False, i % N) for i in range(L.n)], Cn)


# ---- 2. and 3. decode ------------------------------------------------------------------------------------------------------------

def expectation(L, W, H, Cn, is16, rows, flags, origins=(0, 0), pixels_max=-1, kind=None, scale=1.0, bias=0.0, order="rgb"):
    """CR.expectation with a flip per window: -> (the buffer's fill, the buffer the call must leave, which rows are readable)"""
    ch, cw = L.shape[-3], L.shape[-2]
    buf = floats.fill_bits(L.samples, kind) if kind else V.pattern(L.samples, is16)
    want = buf.copy()
    readable = []
    for w, data, (x0, y0), f in zip(L.np_windows(want), rows, CR.origins_list(origins, L.n), flags):
        ref = V.oracle_decode(data, W, H, Cn, is16, pixels_max)
        readable.append(ref is not None)
        if ref is None:
            continue
        part = ref[y0:y0 + ch, x0:x0 + cw]
        if part.size:
            if kind:
                part = floats.reference(part, kind, scale, bias, order)
            elif order == "bgr" and Cn == 3:
                part = part[..., ::-1]
            flip.place(w, part, f)
    return buf, want, readable


def decode(ctx, L, tbuf, streams, lens, fs, size=None, origins=None, kind=None, **kw):
    """the call for L's kind: a list, or a grid through the keyword of decode_view / decode_view_float / decode_view_crop"""
    if isinstance(L, LG.Scatter):
        return ctx.decode_view_list(streams, lens, L.t_windows(tbuf), size, origins, flip=fs, **kw)
    if size is not None:
        return ctx.decode_view_crop(streams, lens, L.t_view(tbuf), size, origins, flip=fs, **kw)
    if kind:
        return ctx.decode_view_float(streams, lens, L.t_view(tbuf), flip=fs, **kw)
    return ctx.decode_view(streams, lens, L.t_view(tbuf), flip=fs, **kw)


def check_decode(ctx, L, W, H, Cn, is16, rows, fs, pixels_max=-1, kind=None, scale=1.0, bias=0.0, size=None, origins=None, order="rgb", **call):
    flags = flags_of(fs, L.n)
    buf, want, readable = expectation(L, W, H, Cn, is16, rows, flags, origins or (0, 0), pixels_max, kind, scale, bias, order)
    streams, lens = F.upload(ctx, rows)
    if kind:
        tbuf, raw = floats.to_device_floats(ctx.device, buf, kind)
        more = dict(scale=scale, bias=bias, maxval=M16 if is16 else 255)
    else:
        tbuf = raw = V.to_device(ctx, buf)
        more = dict(maxval=M16 if is16 else None)
    infos = decode(ctx, L, tbuf, streams, lens, fs, size, origins, kind, levels_max=deep.levels_max(W, H, pixels_max), order=order, **more, **call)
    assert [I.status == 0 for I in infos] == readable
    got = floats.bits_of(raw) if kind else V.to_host(raw, is16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"flags {fs}: {bad.size} samples differ, first at {bad[:5]} of {L.samples} (strides {L.strides}): got {got[bad[:5]]}, want {want[bad[:5]]}"
    return infos


@quads
@hows
@pytest.mark.parametrize("layout", list(LG.LAYOUTS))
def test_flipped_decode_writes_the_flipped_windows_and_nothing_else(ctx, layout, how, nudge):
    """whole streams: every layout x flags x (grid | list) x (quad | off), shapes by a seeded choice"""
    Cn, is16, kw, call = LG.LAYOUTS[layout]
    rng = random.Random(f"dec {layout} {how} {nudge}")
    for k, fs in enumerate(FLAGSETS):
        W, H = shape_for(rng, k)
        print(fs, W, H)
        check_decode(ctx, windows_of(how, W, H, Cn, nudge, **kw), W, H, Cn, is16, CR.whole_rows(W, H, Cn, is16, N), fs, **call)


@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_flipped_decode_of_every_shape(ctx, wh):
    """each shape under the mixed flags — whole, cut, the two mixed, and under a level cap — RGB on a grid and gray as a list"""
    W, H = wh
    for Cn, how in ((3, "grid"), (1, "list")):
        L = windows_of(how, W, H, Cn, None)
        for name, rows, pixels_max in V.decode_cases(W, H, Cn, False, L.n):
            print(name)
            check_decode(ctx, L, W, H, Cn, False, rows, flip.MIXED, pixels_max)


@quads
@hows
@pytest.mark.parametrize("kind", floats.KINDS)
@pytest.mark.parametrize("layout", ["gray", "planar", "rgb", "planar-bgr"])
def test_flipped_decode_into_float_windows(ctx, layout, kind, how, nudge):
    W, H = 72, 68
    Cn, is16, kw, call = LG.LAYOUTS[layout]
    L = windows_of(how, W, H, Cn, nudge, **kw)
    scale, bias = floats.SETS["imagenet"](255)
    rows = CR.whole_rows(W, H, Cn, False, L.n)
    rows[4] = V.cut(*V.oracle_encode(W, H, Cn, False, 4))
    for fs in FLAGSETS:
        check_decode(ctx, L, W, H, Cn, False, rows, fs, kind=kind, scale=scale, bias=bias, **call)


def test_flipped_decode_of_deep_streams_into_float16(ctx):
    W, H = 72, 68
    L = windows_of("grid", W, H, 3, None, planar=True)
    scale, bias = floats.SETS["imagenet"](M16)
    check_decode(ctx, L, W, H, 3, True, CR.whole_rows(W, H, 3, True, L.n), flip.MIXED, kind="float16", scale=scale, bias=bias)


# (sink, channels, keywords of the windows, keywords of check_decode)
SINKS = {
    "gray-u8": (1, {}, {}),
    "rgb-u8": (3, {}, {}),
    "planar-f16": (3, dict(planar=True), dict(kind="float16")),
    "rgbx": (3, dict(step=4), dict(stepped=True)),
}


def sink_call(sink):
    Cn, kw, call = SINKS[sink]
    call = dict(call)
    if "kind" in call:
        call["scale"], call["bias"] = floats.SETS["imagenet"](255)
    return Cn, kw, call


@hows
@pytest.mark.parametrize("sink", list(SINKS))
@pytest.mark.parametrize("wh", [(520, 264), (263, 135)], ids=lambda wh: "%dx%d" % wh)
def test_reduced_pictures_lie_in_their_flipped_corners(ctx, wh, sink, how):
    """stairs (a picture of every size in one batch, whole ones too) and one short stream among whole ones"""
    W, H = wh
    Cn, kw, call = sink_call(sink)
    L = windows_of(how, W, H, Cn, None, **kw)
    for name, rows, pixels_max in levels.level_cases(W, H, Cn, False, L.n, names=("stairs", "one short", "short first")):
        for fs in FLAGSETS:
            print(name, fs)
            check_decode(ctx, L, W, H, Cn, False, rows, fs, pixels_max, **call)


@hows
def test_an_unreadable_stream_leaves_its_flipped_window_untouched(ctx, how):
    W, H, Cn = 72, 68, 3
    L = windows_of(how, W, H, Cn, None)
    rows = CR.whole_rows(W, H, Cn, False, L.n)
    rows[3] = rows[3][:7]
    for fs in FLAGSETS:
        infos = check_decode(ctx, L, W, H, Cn, False, rows, fs)
        assert [I.status for I in infos] == [0, 0, 0, 1, 0]


SWITCHES = [("decode_parts", 2), ("decode_parts", 4), ("one_stream", 1)]


@pytest.mark.parametrize("name,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
@pytest.mark.parametrize("sink,W,H", [("rgb-u8", 263, 135), ("planar-f16", 520, 264), ("gray-u8", 520, 264), ("rgbx", 263, 135)])
def test_reduced_flipped_pictures_under_the_decoder_switches(ctx, opts, sink, W, H, name, value):
    """the parts of a batch start at entries of the table other than the first, and finish pictures one by one"""
    opts.set(name, value)
    Cn, kw, call = sink_call(sink)
    for how in ("grid", "list"):
        L = windows_of(how, W, H, Cn, None, n=8, **kw)
        flags = [3, 0, 1, 2, 2, 1, 3, 0]
        for cname, rows, pixels_max in levels.level_cases(W, H, Cn, False, L.n, names=("stairs", "one short")):
            print(how, cname)
            if cname == "stairs":
                rows = rows[:5] + [rows[5][:7]] + rows[6:]   # (and a stream with status 1 in the middle)
            check_decode(ctx, L, W, H, Cn, False, rows, flags, pixels_max, **call)


@pytest.mark.parametrize("rows_per_wave", [4, 64])
def test_flips_under_lift_rows(ctx, opts, rows_per_wave):
    W, H, Cn = 520, 264, 3
    opts.set("lift_rows", rows_per_wave)
    L = windows_of("list", W, H, Cn, None)
    rows = levels.level_cases(W, H, Cn, False, L.n, names=("stairs",))[0][1]
    check_decode(ctx, L, W, H, Cn, False, rows, flip.MIXED)
    check_encode(ctx, L, W, H, Cn, False, flip.MIXED)


# ---- 4. crop with flips ----------------------------------------------------------------------------------------------------------

ROUTES = (1, 2)


@pytest.mark.parametrize("name,cw,ch,origin", CR.REDUCED, ids=[r[0] for r in CR.REDUCED])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_flipped_crops_of_reduced_pictures(ctx, opts, Cn, name, cw, ch, origin):
    """pictures that come out at 132x68; crops inside, across the edges and outside, with origins and flags of their own"""
    W, H = 263, 135
    T = levels.levels_of(W, H)
    rows = [levels.prefix_for_level(levels.stream(W, H, Cn, False, i), W, H, Cn, T - 2) for i in range(N)]
    origins = [(origin[0] + i, origin[1] + (2 * i) % 3) for i in range(N)]
    for route in ROUTES:
        opts.set("crop_route", route)
        for how in ("grid", "list"):
            check_decode(ctx, windows_of(how, cw, ch, Cn, None), W, H, Cn, False, rows, flip.MIXED, size=(W, H), origins=origins)
    check_decode(ctx, windows_of("list", cw, ch, Cn, 2), W, H, Cn, False, rows, 3, size=(W, H), origins=origins)


GENERAL = [pytest.param(W, H, Cn, c, id="%dx%d-%s-%dx%d@%d,%d" % ((W, H, "rgb" if Cn == 3 else "gray") + c))
           for W, H, Cn in ((130, 67, 3), (37, 53, 1), (72, 68, 3), (64, 64, 1)) for c in CR.general_crops(W, H)]


@pytest.mark.parametrize("W,H,Cn,c", GENERAL)
def test_flipped_crops_with_origins_of_their_own(ctx, opts, W, H, Cn, c):
    cw, ch, x0, y0 = c
    origins = [(max(0, x0 - i), max(0, y0 - (2 * i) % 5)) for i in range(N)]
    rows = CR.whole_rows(W, H, Cn, False, N)
    for route in ROUTES:
        opts.set("crop_route", route)
        for how in ("grid", "list"):
            check_decode(ctx, windows_of(how, cw, ch, Cn, None), W, H, Cn, False, rows, flip.MIXED, size=(W, H), origins=origins)


def test_a_loaders_crop_and_flip_into_planar_float16(ctx):
    """the step the feature is for: decode, crop, convert, normalise and mirror some pictures, in one call into [N,3,h,w]"""
    import torch

    W, H, cw, ch, n = 263, 135, 96, 64, N
    scale, bias = floats.SETS["imagenet"](255)
    batch = torch.zeros((n, 3, ch, cw), dtype=torch.float16, device=ctx.device)
    rows = CR.whole_rows(W, H, 3, False, n)
    streams, lens = F.upload(ctx, rows)
    origins = CR.spread(n, 31, 17)
    mask = [0, 1, 1, 0, 1]
    ctx.decode_view_crop(streams, lens, batch.permute(0, 2, 3, 1), (W, H), origins, scale=scale, bias=bias, flip=mask)
    got = batch.view(torch.int16).cpu().numpy().view(np.uint16)
    for i, (x0, y0) in enumerate(origins):
        part = floats.reference(V.oracle_decode(rows[i], W, H, 3, False)[y0:y0 + ch, x0:x0 + cw], "float16", scale, bias)
        assert (got[i] == flip.in_memory(part, mask[i]).transpose(2, 0, 1)).all(), i


# ---- 5. equivalences -------------------------------------------------------------------------------------------------------------

def _p(t):
    return C.c_void_p(t.data_ptr())


def raw_encode_flip(ctx, v, step, arr, flips, W, H, n, out, info, flip_all=0, fmt=None, order=0):
    fl = None if flips is None else (C.c_ubyte * n)(*flips)
    return ctx.lib.dwtx_encode_view_flip(ctx.h, C.byref(v), step, order, fmt, arr, flip_all, fl, W, H, n, 0, _p(out), out.shape[1], _p(info)), fl


def raw_decode_flip(ctx, v, step, arr, flips, W, H, n, streams, lens, infos, cw=None, ch=None, org=None, flip_all=0, fmt=None, order=0):
    fl = None if flips is None else (C.c_ubyte * n)(*flips)
    return ctx.lib.dwtx_decode_view_flip(ctx.h, _p(streams), streams.shape[1], _p(lens), W, H, n, -1, C.byref(v), step, order, fmt,
                                         W if cw is None else cw, H if ch is None else ch, org, arr, flip_all, fl, C.cast(infos, C.c_void_p)), fl


def view_of(L, tbuf, Cn, sample_bytes=1, maxval=255):
    """the dwtx_view of a gridded() layout (dev set) or of a scatter (dev NULL) and the pointer array of the latter"""
    import dwt_amd

    if isinstance(L, LG.Scatter):
        cs = L.strides[2] if L.strides[1] == 1 and Cn == 3 else 0
        v = dwt_amd.View(None, sample_bytes, Cn, maxval, 0, L.strides[0], 0, 0, cs)
        return v, (C.c_void_p * L.n)(*[tbuf.data_ptr() + o * sample_bytes for o in L.offs])
    cs = L.strides[3] if L.strides[2] == 1 and Cn == 3 else 0
    return dwt_amd.View(tbuf.data_ptr() + L.off * sample_bytes, sample_bytes, Cn, maxval, 0, L.strides[1], L.strides[0], 0, cs), None


@hows
@pytest.mark.parametrize("W,H,Cn", [(72, 68, 3), (263, 135, 1)])
def test_all_flags_zero_is_the_unflipped_call(ctx, W, H, Cn, how):
    """flags 0 — one for all, or a list of zeros — against the list call / the grid call: streams, infos and buffer, bit for bit"""
    import torch

    import dwt_amd

    L = windows_of(how, W, H, Cn, None)
    buf = V.pattern(L.samples, False)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = V.picture(W, H, Cn, False, i)
    src = V.to_device(ctx, buf)
    stride = ctx.lib.dwtx_encode_bound(W, H, Cn)
    plain_out, plain_info = (ctx.encode_view_list(L.t_windows(src)) if how == "list" else ctx.encode_view(L.t_view(src)))
    v, arr = view_of(L, src, Cn)
    for flips in (None, [0] * L.n):
        out = torch.zeros((L.n, stride), dtype=torch.uint8, device=ctx.device)
        info = torch.zeros((L.n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
        rc, _ = raw_encode_flip(ctx, v, 0, arr, flips, W, H, L.n, out, info)
        assert rc == 0, ctx.lib.dwtx_last_error()
        ctx.sync()
        lens = ctx.stream_lengths(plain_info).cpu().numpy()
        assert torch.equal(info, plain_info) and all(torch.equal(out[i, :lens[i]], plain_out[i, :lens[i]]) for i in range(L.n))
    rows = CR.whole_rows(W, H, Cn, False, L.n)
    rows[1] = V.cut(*V.oracle_encode(W, H, Cn, False, 1))
    rows[3] = rows[3][:7]
    streams, lens = F.upload(ctx, rows)
    fill = V.pattern(L.samples, False)
    a = V.to_device(ctx, fill)
    ia = ctx.decode_view_list(streams, lens, L.t_windows(a)) if how == "list" else ctx.decode_view(streams, lens, L.t_view(a))
    for flips in (None, [0] * L.n):
        b = V.to_device(ctx, fill)
        v, arr = view_of(L, b, Cn)
        infos = (dwt_amd.DecodeInfo * L.n)()
        rc, _ = raw_decode_flip(ctx, v, 0, arr, flips, W, H, L.n, streams, lens, infos)
        assert rc == 0, ctx.lib.dwtx_last_error()
        assert torch.equal(a, b) and not torch.equal(a, V.to_device(ctx, fill))
        assert [CR.record(I) for I in ia] == [CR.record(I) for I in infos]


@hows
@pytest.mark.parametrize("layout,W,H", [("rgb", 72, 68), ("gray", 256, 256), ("planar", 263, 135), ("bgrx", 72, 68), ("rgb16", 72, 68)])
def test_decode_with_flags_then_encode_with_the_same_flags_gives_the_streams_back(ctx, layout, W, H, how):
    Cn, is16, kw, call = LG.LAYOUTS[layout]
    L = windows_of(how, W, H, Cn, None, **kw)
    rows = CR.whole_rows(W, H, Cn, is16, L.n)
    streams, lens = F.upload(ctx, rows)
    for fs in FLAGSETS:
        tbuf = V.to_device(ctx, V.pattern(L.samples, is16))
        decode(ctx, L, tbuf, streams, lens, fs, maxval=M16 if is16 else None, **call)
        out, info = encode(ctx, L, tbuf, fs, **call)
        assert EI._streams_of(ctx, out, info) == rows, fs


def test_host_info_is_the_plain_decodes(ctx):
    W, H, Cn = 263, 135, 3
    T = levels.levels_of(W, H)
    L = windows_of("grid", W, H, Cn, None, n=4)
    rows = [levels.stream(W, H, Cn, False, i) for i in range(4)]
    rows[1] = V.cut(*V.oracle_encode(W, H, Cn, False, 1))
    rows[2] = levels.prefix_for_level(rows[2], W, H, Cn, T - 2)
    rows[3] = rows[3][:7]
    streams, lens = F.upload(ctx, rows)
    plain = ctx.decode_view(streams, lens, L.t_view(V.to_device(ctx, V.pattern(L.samples, False))))
    for fs in (1, 2, [3, 0, 2, 1]):
        got = ctx.decode_view(streams, lens, L.t_view(V.to_device(ctx, V.pattern(L.samples, False))), flip=fs)
        assert [CR.record(I) for I in got] == [CR.record(I) for I in plain]


# ---- 6. contracts ----------------------------------------------------------------------------------------------------------------

def test_the_host_arrays_may_be_overwritten_as_soon_as_the_call_returns(ctx):
    import torch

    import dwt_amd

    W, H, Cn = 72, 68, 1
    L = LG.scatter(W, H, Cn)
    flags = flip.MIXED
    buf = V.pattern(L.samples, False)
    for i, w in enumerate(L.np_windows(buf)):
        w[...] = flip.in_memory(V.picture(W, H, Cn, False, i), flags[i])
    tbuf = V.to_device(ctx, buf)
    decoy = torch.zeros(L.samples, dtype=torch.uint8, device=ctx.device)
    v, arr = view_of(L, tbuf, Cn)
    stride = ctx.lib.dwtx_encode_bound(W, H, Cn)
    out = torch.zeros((L.n, stride), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros((L.n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
    busy = ctx.synth_pixels(16, 1024, 1024, 1)
    ctx.encode_device(busy)   # (work on the context's stream that the asynchronous flipped encode is queued behind)
    rc, fl = raw_encode_flip(ctx, v, 0, arr, flags, W, H, L.n, out, info)
    for i in range(L.n):
        arr[i] = decoy.data_ptr()
        fl[i] = 3 - flags[i]
    assert rc == 0, ctx.lib.dwtx_last_error()
    ctx.sync()
    wants = [V.oracle_encode(W, H, Cn, False, i) for i in range(L.n)]
    LG.check_streams(out, info, wants, Cn)
    # the decode: its windows, its origins and its flags
    cw, ch = 40, 30
    D = LG.scatter(cw, ch, Cn)
    origins = [(3 * i, 2 * i + 1) for i in range(D.n)]
    rows = [w for w, _ in wants]
    fill, want, _ = expectation(D, W, H, Cn, False, rows, flags, origins)
    dbuf = V.to_device(ctx, fill)
    streams, lens = F.upload(ctx, rows)
    v, arr = view_of(D, dbuf, Cn)
    org = (C.c_int * (2 * D.n))(*[c for o in origins for c in o])
    infos = (dwt_amd.DecodeInfo * D.n)()
    rc, fl = raw_decode_flip(ctx, v, 0, arr, flags, W, H, D.n, streams, lens, infos, cw, ch, org)
    for i in range(D.n):
        arr[i] = decoy.data_ptr()
        org[2 * i] = org[2 * i + 1] = 0
        fl[i] = 3 - flags[i]
    assert rc == 0, ctx.lib.dwtx_last_error()
    ctx.sync()
    assert (V.to_host(dbuf, False) == want).all() and not decoy.any()


def test_flipped_and_unflipped_calls_follow_one_another_on_one_context(ctx):
    """what a call leaves behind — the table's slot with flags in its entries, the staging buffer and its event — must not show in
    the next one: every result is the oracle's"""
    import dwt_amd

    c = dwt_amd.Context(0)
    try:
        W, H, Cn = 72, 68, 3
        S5, S4, G = LG.scatter(W, H, Cn), LG.scatter(W, H, Cn, n=4, nudge=1), gridded(W, H, Cn)
        rows = CR.whole_rows(W, H, Cn, False, 5)
        for _ in range(2):
            LG.check_decode(c, S5, W, H, Cn, False, rows)                 # unflipped, listed
            check_decode(c, S5, W, H, Cn, False, rows, 3)                  # flipped right after it, the same windows
            LG.check_decode(c, S4, W, H, Cn, False, rows[1:])              # and the reverse: entries that carried flags
            check_decode(c, G, W, H, Cn, False, rows, flip.MIXED)
            V.check_decode(ctx, G, W, H, Cn, False, rows, view_ctx=c)      # a plain grid call
            check_encode(c, S5, W, H, Cn, False, flip.MIXED)
            LG.check_encode(c, S5, W, H, Cn, False)
            check_encode(c, G, W, H, Cn, False, 2)
            LG.check_encode(c, S4, W, H, Cn, False, pics=[3, 1, 0, 2])
    finally:
        c.close()


@quads
def test_flipped_windows_more_than_2_to_the_32_samples_apart(nudge):
    """LG's far windows with flags 3: the origin of the far window's picture lies at its LAST sample, beyond 2^32"""
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
        ghost = frame[near + (far - near) % (1 << 32):][:size]
        pics = [torch.from_numpy(V.picture(W, H, Cn, False, i)).to(c.device).flip(0, 1) for i in range(2)]
        rows = CR.whole_rows(W, H, Cn, False, 2)
        streams, lens = F.upload(c, rows)
        infos = c.decode_view_list(streams, lens, wins, flip=3)
        assert all(I.status == 0 for I in infos)
        assert torch.equal(wins[0], pics[0]) and torch.equal(wins[1], pics[1])
        assert bool((ghost == FILL).all()) and bool((frame[near + size:near + size + 4096] == FILL).all())
        assert bool((frame[far - 4096:far] == FILL).all()) and bool((frame[far + size:] == FILL).all())
        ghost.copy_(pics[1].reshape(-1))
        out, info = c.encode_view_list(wins, flip=[3, 3])
        LG.check_streams(out, info, [V.oracle_encode(W, H, Cn, False, i) for i in range(2)], Cn)
    finally:
        c.close()
        frame = wins = ghost = None
        torch.cuda.empty_cache()


def test_alpha_and_padding_survive_a_flipped_rgb_decode(ctx):
    """an RGBA stack and grid: the fourth byte of every pixel, the rows' padding and the frame around the windows keep their fill"""
    W, H = 72, 68
    for L in (S.sstack(W, H, 3, 4, n=5), S.sgrid(W, H, 3, 4, rows=2, cols=3)):
        rows = CR.whole_rows(W, H, 3, False, L.n)
        rows[2] = V.cut(*V.oracle_encode(W, H, 3, False, 2))
        for fs in (1, 2, 3, (flip.MIXED + [2])[:L.n]):
            check_decode(ctx, L, W, H, 3, False, rows, fs, stepped=True)
            check_decode(ctx, L, W, H, 3, False, rows, fs, stepped=True, order="bgr")


# ---- 7. tiles --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", ["y", "xy", "x"])
def test_a_flipped_frame_round_trips_through_tiles(ctx, f):
    import torch

    from dwt_amd import tiles

    FW, FH, tile = 150, 100, 64
    upright = orc.synth(FW, FH, 3, 11, 0)
    mem = np.ascontiguousarray(flip.in_memory(upright, dwt_amd_flag(f)))
    frame = torch.from_numpy(mem).to(ctx.device)
    want = tiles.encode_frame(ctx, torch.from_numpy(upright).to(ctx.device), tile)
    got = tiles.encode_frame(ctx, frame, tile, flip=f)
    assert len(got) == len(want) == 4
    for (g, streams, lens, info), (wg, wstreams, wlens, winfo) in zip(got, want):
        assert bytes(g) == bytes(wg) and torch.equal(lens, wlens) and torch.equal(info, winfo)
        assert EI._streams_of(ctx, streams, info) == EI._streams_of(ctx, wstreams, winfo)
        for i, s in enumerate(EI._streams_of(ctx, streams, info)):   # tile (i // cols, i % cols) of the upright frame
            y, x = g.y0 + (i // g.cols) * g.H, g.x0 + (i % g.cols) * g.W
            assert s == orc.encode(np.ascontiguousarray(upright[y:y + g.H, x:x + g.W]))[0], (f, i)
    into = torch.full_like(frame, 0x5A)
    infos = tiles.decode_frame(ctx, got, into, flip=f)
    assert all(I.status == 0 for group in infos for I in group)
    assert torch.equal(into, frame)


def dwt_amd_flag(f):
    import dwt_amd

    return dwt_amd.FLIPS[f]


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------

def test_refused_flipped_calls_leave_everything_as_it_was(ctx):
    import torch

    import dwt_amd

    W, H, Cn, n = 72, 68, 1, 3
    L = LG.scatter(W, H, Cn, n=n)
    fill = V.pattern(L.samples, False)
    tbuf = V.to_device(ctx, fill)
    rows = CR.whole_rows(W, H, Cn, False, n)
    streams, lens = F.upload(ctx, rows)
    v, arr = view_of(L, tbuf, Cn)
    overlap = (C.c_void_p * n)(arr[0], arr[0] + 5, arr[2])
    G = gridded(W, H, Cn, n=n)
    gbuf = V.to_device(ctx, V.pattern(G.samples, False))
    gv, _ = view_of(G, gbuf, Cn)
    gv_overlap, _ = view_of(G, gbuf, Cn)
    gv_overlap.image_stride = (H - 1) * G.strides[1] + W - 1
    stride = ctx.lib.dwtx_encode_bound(W, H, Cn)
    out = torch.zeros((n, stride), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()
    C.memset(infos, 0x5A, C.sizeof(infos))
    before = bytes(infos)
    dec = lambda v, arr, flips, flip_all=0: raw_decode_flip(ctx, v, 0, arr, flips, W, H, n, streams, lens, infos, flip_all=flip_all)[0]   # noqa: E731
    enc = lambda v, arr, flips, flip_all=0: raw_encode_flip(ctx, v, 0, arr, flips, W, H, n, out, info, flip_all=flip_all)[0]   # noqa: E731
    bad = [
        ("a flag of 4 for all", lambda call: call(v, arr, None, 4), "4"),
        ("a negative flag", lambda call: call(v, arr, None, -2), "-2"),
        ("a flag of 4 in the list", lambda call: call(v, arr, [0, 4, 1]), "window 1"),
        ("a flag of 4 on a grid", lambda call: call(gv, None, [3, 2, 4]), "window 2"),
        ("flip together with host_flips", lambda call: call(v, arr, [0, 1, 2], 1), "host_flips"),
        ("flip together with host_flips of zeros", lambda call: call(gv, None, [0, 0, 0], 2), "host_flips"),
    ]
    for what, fn, word in bad:
        for call in (dec, enc):
            assert fn(call) == ERR_ARG, what
            assert word.encode() in ctx.lib.dwtx_last_error(), (what, ctx.lib.dwtx_last_error())
    for what, fn, word in [("a decode list that overlaps", lambda: dec(v, overlap, [1, 2, 3]), "disjoint"),
                           ("a decode grid that overlaps", lambda: dec(gv_overlap, None, None, 3), "overlap"),
                           ("a NULL window", lambda: dec(v, (C.c_void_p * n)(arr[0], None, arr[2]), [1, 2, 3]), "NULL")]:
        assert fn() == ERR_ARG, what
        assert word.encode() in ctx.lib.dwtx_last_error(), (what, ctx.lib.dwtx_last_error())
    ctx.sync()
    assert bytes(infos) == before
    assert (V.to_host(tbuf, False) == fill).all() and (V.to_host(gbuf, False) == V.pattern(G.samples, False)).all()
    assert not out.any() and not info.any()
    # an encode may read windows that overlap, and the same arguments with good flags are taken
    assert enc(v, overlap, [1, 2, 3]) == 0 and dec(v, arr, [1, 2, 3]) == 0 and dec(gv, None, None, 3) == 0
    ctx.sync()


def test_bad_flip_keywords_raise_before_any_device_call(ctx):
    W, H, Cn = 72, 68, 1
    L = gridded(W, H, Cn)
    buf = V.pattern(L.samples, False)
    tbuf = V.to_device(ctx, buf)
    streams, lens = F.upload(ctx, CR.whole_rows(W, H, Cn, False, L.n))
    for bad in (4, "z", [0, 1], [0, 1, 2, 3, 4]):
        with pytest.raises(ValueError):
            ctx.decode_view(streams, lens, L.t_view(tbuf), flip=bad)
        with pytest.raises(ValueError):
            ctx.encode_view(L.t_view(tbuf), flip=bad)
        with pytest.raises(ValueError):
            ctx.decode_view_list(streams, lens, [w for w in L.t_view(tbuf)], flip=bad)
        with pytest.raises(ValueError):
            ctx.decode_view_crop(streams, lens, L.t_view(tbuf)[:, :20, :20], (W, H), flip=bad)
    assert (V.to_host(tbuf, False) == buf).all()
