"""GPU: crop decode (dwtx_decode_view_crop, include/dwtx.h) — a window of each picture written straight into a view.

The yardstick is the oracle's picture, sliced: orc.decode for bytes, deep.deep_decode for 16-bit samples (maxval 4095);
float expectations follow from the integers as tests/floats.py has them.  Destinations are built as in
tests/test_views_gpu.py — a patterned flat buffer plus a layout whose windows have the crop's size — and after the call the
WHOLE buffer must equal the expectation: the slice in each window's corner, the pattern everywhere else.  Every case runs
under DWTX_OPT_CROP_ROUTE 1 (windowed levels), 2 (whole inverse, then a gather) and 0 (automatic).  Every comparison is
exact."""
import ctypes as C

import numpy as np
import pytest

import deep
import floats
import levels
import orc
import test_float_gpu as F
import test_planar_gpu as P
import test_step_gpu as S
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
M16 = V.M16
ROUTES = (1, 2, 0)


def origins_list(origins, n):
    return [tuple(origins)] * n if not hasattr(origins[0], "__len__") else [tuple(o) for o in origins]


def expectation(L, W, H, Cn, is16, rows, origins, pixels_max=-1, kind=None, scale=1.0, bias=0.0, order="rgb"):
    """-> (the buffer's fill, the buffer the call must leave, the rows' statuses as the oracle sees them)"""
    ch, cw = L.shape[-3], L.shape[-2]
    buf = floats.fill_bits(L.samples, kind) if kind else V.pattern(L.samples, is16)
    want = buf.copy()
    readable = []
    for w, data, (x0, y0) in zip(L.np_windows(want), rows, origins_list(origins, L.n)):
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
            w[:part.shape[0], :part.shape[1]] = part
    return buf, want, readable


def check_crop(ctx, opts, L, W, H, Cn, is16, rows, origins, pixels_max=-1, kind=None, scale=1.0, bias=0.0, stepped=False, order="rgb", routes=ROUTES):
    """rows: one stream per window of L, whose windows are the crop.  origins: one (x0, y0) or one per window."""
    buf, want, readable = expectation(L, W, H, Cn, is16, rows, origins, pixels_max, kind, scale, bias, order)
    streams, lens = F.upload(ctx, rows)
    infos = None
    for route in routes:
        opts.set("crop_route", route)
        if kind:
            tbuf, raw = floats.to_device_floats(ctx.device, buf, kind)
            more = dict(scale=scale, bias=bias, maxval=M16 if is16 else 255)
        else:
            tbuf = raw = V.to_device(ctx, buf)
            more = dict(maxval=M16 if is16 else None)
        infos = ctx.decode_view_crop(streams, lens, L.t_view(tbuf), (W, H), origins, levels_max=deep.levels_max(W, H, pixels_max),
                                     stepped=stepped, order=order, **more)
        assert [I.status == 0 for I in infos] == readable
        got = floats.bits_of(raw) if kind else V.to_host(raw, is16)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"route {route}: {bad.size} samples differ, first at {bad[:5]} of {L.samples} (view offset {L.off}, strides {L.strides}): "
                               f"got {got[bad[:5]]}, want {want[bad[:5]]}")
    return infos


def whole_rows(W, H, Cn, is16, n, first=0):
    return [V.oracle_encode(W, H, Cn, is16, first + i)[0] for i in range(n)]


# ---- shapes and crops ------------------------------------------------------------------------------------------------------

def corners(W, H):
    return [(1, 1, 0, 0), (1, 1, W - 1, 0), (1, 1, 0, H - 1), (1, 1, W - 1, H - 1)]


def general_crops(W, H):
    """for the shapes without crops of their own: the whole picture, one pixel in the far corner, a window with odd origin
    and sides, and one that touches the right and bottom edges"""
    return [(W, H, 0, 0), (1, 1, W - 1, H - 1), (W // 2 + 1, H // 2 + 1, (W // 3) | 1, (H // 3) | 1), (7, 5, W - 7, H - 5)]


# (W, H, channels, [(cw, ch, x0, y0)]): 263x135 general whole; 200x100 at (31, 17) crosses a 62-pair strip at two levels; 7x9 at
# (255, 125) touches the odd right and bottom edges, the `frozen` sample; 256x256: a shape whose plain decode uses 16-bit rings
# and the two-level kernel; 64x64 and 8x8: all tail
CASES = [
    (263, 135, (1, 3), [(263, 135, 0, 0)] + corners(263, 135) + [(200, 100, 31, 17), (7, 9, 255, 125)]),
    (520, 264, (3,), [(400, 200, 61, 33)]),
    (256, 256, (1,), [(96, 64, 80, 96)]),
    (130, 67, (1, 3), general_crops(130, 67)),
    (37, 53, (1, 3), general_crops(37, 53)),
    (72, 68, (1, 3), general_crops(72, 68)),
    (64, 64, (1, 3), general_crops(64, 64)),
    (8, 8, (1, 3), [(1, 1, 3, 4), (8, 8, 0, 0)]),
]
CASE_PARAMS = [pytest.param(W, H, Cn, c, id="%dx%d-%s-%dx%d@%d,%d" % ((W, H, "rgb" if Cn == 3 else "gray") + c))
               for W, H, Cns, crops in CASES for Cn in Cns for c in crops]


@pytest.mark.parametrize("W,H,Cn,c", CASE_PARAMS)
def test_crop_writes_the_slice_and_nothing_else(ctx, opts, W, H, Cn, c):
    cw, ch, x0, y0 = c
    L = V.stack(cw, ch, Cn, n=2)
    check_crop(ctx, opts, L, W, H, Cn, False, whole_rows(W, H, Cn, False, 2), (x0, y0))


@pytest.mark.parametrize("W,H,Cn", [(263, 135, 3), (256, 256, 1)])
def test_every_picture_has_its_own_origin(ctx, opts, W, H, Cn):
    cw, ch = 100, 60
    origins = [(0, 0), (1, 0), (0, 1), (1, 1), (W - cw, H - ch), (W - cw - 1, 3)]
    L = V.grid(cw, ch, Cn, rows=2, cols=3)
    check_crop(ctx, opts, L, W, H, Cn, False, whole_rows(W, H, Cn, False, 6), origins)


# ---- sinks -----------------------------------------------------------------------------------------------------------------

def spread(n, x0, y0):
    return [(x0 + i, y0 + 2 * i) for i in range(n)]


@pytest.mark.parametrize("layout", ["stack", "band", "grid"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_crop_into_stack_band_and_grid_windows(ctx, opts, layout, Cn):
    W, H, cw, ch = 263, 135, 40, 30
    L = V.LAYOUTS[layout](cw, ch, Cn)
    check_crop(ctx, opts, L, W, H, Cn, False, whole_rows(W, H, Cn, False, L.n), spread(L.n, 31, 17))


@pytest.mark.parametrize("layout", ["nchw", "chw_grid", "cnhw"])
def test_crop_into_planar_windows(ctx, opts, layout):
    W, H, cw, ch = 263, 135, 40, 30
    L = P.LAYOUTS[layout](cw, ch)
    check_crop(ctx, opts, L, W, H, 3, False, whole_rows(W, H, 3, False, L.n), spread(L.n, 31, 17))


def test_crop_into_rgba_leaves_alpha_and_padding(ctx, opts):
    W, H, cw, ch = 263, 135, 41, 29
    L = S.sstack(cw, ch, 3, 4)
    check_crop(ctx, opts, L, W, H, 3, False, whole_rows(W, H, 3, False, L.n), spread(L.n, 30, 18), stepped=True)
    L = S.sgrid(cw, ch, 1, 2, rows=2, cols=2)   # one plane of a two-sample mosaic
    check_crop(ctx, opts, L, W, H, 1, False, whole_rows(W, H, 1, False, L.n), spread(L.n, 30, 18), stepped=True)


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_crop_into_bgr(ctx, opts, planar):
    W, H, cw, ch = 263, 135, 40, 30
    L = P.nchw(cw, ch) if planar else V.stack(cw, ch, 3)
    check_crop(ctx, opts, L, W, H, 3, False, whole_rows(W, H, 3, False, L.n), spread(L.n, 31, 17), order="bgr")
    L = S.sstack(cw, ch, 3, 4)
    check_crop(ctx, opts, L, W, H, 3, False, whole_rows(W, H, 3, False, L.n), (222, 104), stepped=True, order="bgr")


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", [(263, 135), (256, 256)], ids=lambda wh: "%dx%d" % wh)
def test_crop_of_deep_pictures(ctx, opts, wh, Cn):
    W, H = wh
    cw, ch = 90, 50
    L = V.stack(cw, ch, Cn)
    check_crop(ctx, opts, L, W, H, Cn, True, whole_rows(W, H, Cn, True, L.n), [(0, 0), (83, 41), (W - cw, H - ch)])


@pytest.mark.parametrize("kind", floats.KINDS)
@pytest.mark.parametrize("layout", ["gray-stack", "rgb-stack", "nchw"])
def test_crop_into_float_tensors(ctx, opts, layout, kind):
    W, H, cw, ch = 263, 135, 44, 28
    Cn, make = F.LAYOUTS[layout]
    L = make(cw, ch)
    scale, bias = floats.SETS["imagenet"](255)
    check_crop(ctx, opts, L, W, H, Cn, False, whole_rows(W, H, Cn, False, L.n), spread(L.n, 31, 17), kind=kind, scale=scale, bias=bias)
    check_crop(ctx, opts, L, W, H, Cn, False, whole_rows(W, H, Cn, False, L.n), (W - cw, H - ch), kind=kind, scale=scale, bias=bias, order="bgr",
               routes=(0,))


def test_crop_of_deep_streams_into_float16(ctx, opts):
    W, H, cw, ch = 263, 135, 44, 28
    L = P.nchw(cw, ch)
    scale, bias = floats.SETS["imagenet"](M16)
    check_crop(ctx, opts, L, W, H, 3, True, whole_rows(W, H, 3, True, L.n), spread(L.n, 31, 17), kind="float16", scale=scale, bias=bias)


# ---- streams that are not whole ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_crop_of_cut_streams(ctx, opts, Cn, is16):
    """the cut() prefix: bias and clamps in play, the picture still full size"""
    W, H, cw, ch = 263, 135, 120, 70
    L = V.stack(cw, ch, Cn)
    rows = [V.cut(*V.oracle_encode(W, H, Cn, is16, i)) for i in range(L.n)]
    assert all(V.oracle_decode(r, W, H, Cn, is16).shape[:2] == (H, W) for r in rows)
    check_crop(ctx, opts, L, W, H, Cn, is16, rows, [(0, 0), (71, 33), (W - cw, H - ch)])


# crops of a picture that came out at 132x68: inside it, across its right and bottom edges (only the intersection is
# written), and outside it (nothing is written)
REDUCED = [("inside", 20, 24, (10, 11)), ("across", 30, 20, (121, 57)), ("outside", 30, 20, (140, 70))]


@pytest.mark.parametrize("name,cw,ch,origin", REDUCED, ids=[r[0] for r in REDUCED])
@pytest.mark.parametrize("how", ["stop", "cap"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_crop_of_reduced_pictures(ctx, opts, Cn, how, name, cw, ch, origin):
    W, H = 263, 135
    T = levels.levels_of(W, H)
    assert levels.sizes(W, H)[T - 1] == (132, 68)
    L = V.stack(cw, ch, Cn)
    rows = [levels.stream(W, H, Cn, False, i) for i in range(L.n)]
    pixels_max = -1
    if how == "stop":   # streams that stop one level short
        rows = [levels.prefix_for_level(r, W, H, Cn, T - 2) for r in rows]
    else:               # whole streams under levels_max
        pixels_max = orc.geometry(W, H).pixels[T - 1]
    for r in rows:
        assert V.oracle_decode(r, W, H, Cn, False, pixels_max).shape[:2] == (68, 132)
    check_crop(ctx, opts, L, W, H, Cn, False, rows, origin, pixels_max)


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_crop_of_a_mixed_batch(ctx, opts, Cn):
    """one short stream among whole ones, and a stream with status 1, whose window is left untouched"""
    W, H, cw, ch = 263, 135, 60, 40
    T = levels.levels_of(W, H)
    L = V.grid(cw, ch, Cn, rows=2, cols=3)
    rows = [levels.stream(W, H, Cn, False, i) for i in range(L.n)]
    rows[2] = levels.prefix_for_level(rows[2], W, H, Cn, T - 2)
    rows[4] = rows[4][:7]
    assert V.oracle_decode(rows[4], W, H, Cn, False) is None
    infos = check_crop(ctx, opts, L, W, H, Cn, False, rows, [(101, 47), (0, 0), (101, 47), (W - cw, H - ch), (5, 5), (1, 1)])
    assert infos[4].status == 1 and infos[2].level == T - 2


# ---- switches --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,value", [("decode_parts", 2), ("decode_parts", 4), ("one_stream", 1)])
def test_crop_under_the_decoder_switches(ctx, opts, name, value):
    W, H, Cn, cw, ch = 263, 135, 3, 60, 40
    opts.set(name, value)
    L = V.grid(cw, ch, Cn, rows=2, cols=4)
    rows = whole_rows(W, H, Cn, False, L.n)
    check_crop(ctx, opts, L, W, H, Cn, False, rows, spread(L.n, 90, 40))
    rows[5] = V.cut(*V.oracle_encode(W, H, Cn, False, 5))
    rows[6] = levels.prefix_for_level(levels.stream(W, H, Cn, False, 6), W, H, Cn, levels.levels_of(W, H) - 2)
    check_crop(ctx, opts, L, W, H, Cn, False, rows, spread(L.n, 90, 40))


@pytest.mark.parametrize("rows_per_wave", [4, 64])
def test_crop_under_lift_rows(ctx, opts, rows_per_wave):
    W, H, Cn = 520, 264, 3
    opts.set("lift_rows", rows_per_wave)
    L = V.stack(400, 200, Cn, n=2)
    check_crop(ctx, opts, L, W, H, Cn, False, whole_rows(W, H, Cn, False, 2), [(61, 33), (120, 64)])


def test_a_bad_route_is_refused(ctx, opts):
    W, H, Cn = 72, 68, 1
    L = V.stack(20, 20, Cn)
    streams, lens = F.upload(ctx, whole_rows(W, H, Cn, False, L.n))
    buf = V.pattern(L.samples, False)
    tbuf = V.to_device(ctx, buf)
    opts.set("crop_route", 3)
    import dwt_amd

    with pytest.raises(dwt_amd.DwtxError) as e:
        ctx.decode_view_crop(streams, lens, L.t_view(tbuf), (W, H), (3, 3))
    assert e.value.rc == ERR_ARG and "CROP_ROUTE" in str(e.value)
    assert (V.to_host(tbuf, False) == buf).all()


# ---- records ---------------------------------------------------------------------------------------------------------------

def record(I):
    return [getattr(I, name) if not hasattr(getattr(I, name), "__len__") else list(getattr(I, name)) for name, _ in I._fields_]


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_host_info_is_the_plain_decodes(ctx, opts, Cn):
    W, H, cw, ch = 263, 135, 60, 40
    T = levels.levels_of(W, H)
    full, L = V.stack(W, H, Cn, n=4), V.stack(cw, ch, Cn, n=4)
    rows = [levels.stream(W, H, Cn, False, i) for i in range(4)]
    rows[1] = V.cut(*V.oracle_encode(W, H, Cn, False, 1))
    rows[2] = levels.prefix_for_level(rows[2], W, H, Cn, T - 2)
    rows[3] = rows[3][:7]
    streams, lens = F.upload(ctx, rows)
    plain = ctx.decode_view(streams, lens, full.t_view(V.to_device(ctx, V.pattern(full.samples, False))))
    for route in ROUTES:
        opts.set("crop_route", route)
        got = ctx.decode_view_crop(streams, lens, L.t_view(V.to_device(ctx, V.pattern(L.samples, False))), (W, H), (100, 50))
        for i in range(4):
            assert record(got[i]) == record(plain[i]), (route, i)


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_bad_crops_are_refused_with_a_text_and_nothing_is_written(ctx):
    import dwt_amd

    W, H, Cn, n, cw, ch = 72, 68, 1, 3, 20, 16
    L = V.stack(cw, ch, Cn, n=n)
    streams, lens = F.upload(ctx, whole_rows(W, H, Cn, False, n))
    buf = V.pattern(L.samples, False)
    tbuf = V.to_device(ctx, buf)
    ftbuf, fraw = floats.to_device_floats(ctx.device, floats.fill_bits(L.samples, "float32"), "float32")
    fbits = floats.bits_of(fraw).copy()
    slot, pitch = L.strides[0], L.strides[1]
    infos = (dwt_amd.DecodeInfo * n)()
    lib = ctx.lib

    def view(dev=tbuf.data_ptr() + L.off, sb=1, maxval=255, pitch=pitch, istride=slot):
        return dwt_amd.View(dev, sb, Cn, maxval, 0, pitch, istride, 0, 0)

    def call(v, cw=cw, ch=ch, origins=None, fmt=None, W=W, H=H):
        org = None if origins is None else (C.c_int * (2 * n))(*[c for o in origins for c in o])
        return lib.dwtx_decode_view_crop(ctx.h, C.c_void_p(streams.data_ptr()), streams.shape[1],
                                         C.c_void_p(lens.data_ptr()), W, H, n, -1, C.byref(v), 0, 0, C.byref(fmt) if fmt is not None else None,
                                         cw, ch, org, C.cast(infos, C.c_void_p))

    f32 = dwt_amd.float_format("float32")
    fview = view(dev=ftbuf.data_ptr() + 4 * L.off, sb=4)
    bad = [
        ("a crop wider than the picture", lambda: call(view(), cw=W + 1)),
        ("a crop higher than the picture", lambda: call(view(), ch=H + 1)),
        ("a width of 0", lambda: call(view(), cw=0)),
        ("a height of 0", lambda: call(view(), ch=0)),
        ("a negative x0", lambda: call(view(), origins=[(0, 0), (-1, 0), (0, 0)])),
        ("a negative y0", lambda: call(view(), origins=[(0, 0), (0, 0), (0, -1)])),
        ("a crop beyond the right edge", lambda: call(view(), origins=[(W - cw + 1, 0), (0, 0), (0, 0)])),
        ("a crop beyond the bottom edge", lambda: call(view(), origins=[(0, 0), (0, H - ch + 1), (0, 0)])),
        ("overlapping windows", lambda: call(view(istride=(ch - 1) * pitch + cw - 1), origins=[(1, 1)] * n)),
        ("a pitch below the crop's row", lambda: call(view(pitch=cw - 1, istride=slot), origins=[(1, 1)] * n)),
        ("a float format with 1-byte samples", lambda: call(view(), origins=[(1, 1)] * n, fmt=f32)),
        ("4-byte samples without a float format", lambda: call(fview, origins=[(1, 1)] * n)),
        ("2-byte samples with a float32 format", lambda: call(view(sb=2, maxval=4095), origins=[(1, 1)] * n, fmt=f32)),
        ("a picture below 8 pixels", lambda: call(view(), cw=4, ch=4, W=7)),
    ]
    for what, fn in bad:
        assert fn() == ERR_ARG, what
        assert lib.dwtx_last_error(), what
        ctx.sync()
        assert (V.to_host(tbuf, False) == buf).all(), what
        assert (floats.bits_of(fraw) == fbits).all(), what
    # and the same view with a good crop is taken
    assert call(view(), origins=[(1, 1)] * n) == 0
    assert call(fview, origins=[(1, 1)] * n, fmt=f32) == 0
    ctx.sync()


# ---- the whole picture is the plain call ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", [(256, 256), (263, 135)], ids=lambda wh: "%dx%d" % wh)
def test_the_whole_picture_is_the_plain_call(ctx, opts, wh, Cn):
    """crop == picture with zero origins (given, or left out): the bytes of decode_view, for a wide and a general shape"""
    W, H = wh
    L = V.band(W, H, Cn)
    rows = whole_rows(W, H, Cn, False, L.n)
    rows[1] = V.cut(*V.oracle_encode(W, H, Cn, False, 1))
    streams, lens = F.upload(ctx, rows)
    buf = V.pattern(L.samples, False)
    plain = V.to_device(ctx, buf)
    pinfos = ctx.decode_view(streams, lens, L.t_view(plain))
    for origins in (None, [(0, 0)] * L.n):
        t = V.to_device(ctx, buf)
        infos = ctx.decode_view_crop(streams, lens, L.t_view(t), (W, H), origins)
        assert (t == plain).all()
        assert [record(I) for I in infos] == [record(I) for I in pinfos]
    check_crop(ctx, opts, L, W, H, Cn, False, rows, (0, 0))
