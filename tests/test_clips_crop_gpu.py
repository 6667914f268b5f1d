"""GPU: dwtx_decode_view_clips_crop (include/dwtx.h) — the clips decode with a crop per clip and, with a format, float windows.

The yardstick is the walk on the CPU (tests/clipsx.py).  An integer crop is also held, bit for bit and with its host_info, to the
slice of decode_view_clips on a second, full-size buffer whose windows hold the crop buffer's prefill at the crops' places.  Every
comparison covers the WHOLE destination buffer — prefilled with seeded random samples of the range, or, for float windows, with
floats.fill_bits (NaNs and infinities among them) — so that a base taken from the wrong place, a window written though its clip
was broken, and a sample written outside a window all change the result.  Shapes are delta.SHAPES; layouts are
tests/test_clips_gpu.py's DESTS with crop-sized windows."""
import numpy as np
import pytest

import chain
import clips
import clipsx
import delta
import floats
import history
import levels
import orc
import test_chain_gpu as CG
import test_clips_gpu as TC
import test_delta_gpu as G
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
SHAPES = delta.SHAPES
KINDS = G.KINDS
KIND_NAMES = G.KIND_NAMES
N = TC.N
CROPS = [(56, 40), (33, 21)]
THIN = [(1, 40), (56, 1)]            # one 1-wide and one 1-high crop
CARRY = [(15, 2, 4), (11, 3, 4)]     # (n, period, DWTX_OPT_DECODE_PARTS): tests/test_clips_crop_cpu.py, a carry read and written in one launch


def origins_of(W, H, cw, ch, k, turn=0):
    """k origins, one per clip: both parities in x and in y, (0, 0), and points clamped to the far corner"""
    pts = [(1, 1), (2, 3), (W, H), (0, 0), (6, 5), (3, 2), (W, 4), (5, H)]
    return [(min(x, W - cw), min(y, H - ch)) for x, y in (pts[(i + turn) % len(pts)] for i in range(k))]


def test_the_origins_meet_both_parities_and_the_far_corner():
    W, H = 132, 72
    o = origins_of(W, H, 56, 40, 8)
    assert {(x % 2, y % 2) for x, y in o} == {(0, 0), (0, 1), (1, 0), (1, 1)} and (W - 56, H - 40) in o
    assert len(set(origins_of(W, H, 33, 21, 3))) == 3 and len(set(origins_of(W, H, 33, 21, 3, 2))) == 3


def check_infos(datas, infos, W, H, Cn):
    T = orc.geometry(W, H).levels
    for i, (data, I) in enumerate(zip(datas, infos)):
        r = clipsx.cropped(data, W, H, Cn, 0, 0, 1, 1)
        if r is None:
            assert I.status != 0, i
        else:
            assert I.status == 0 and (I.level == T - 1) == (r is not clipsx.UNTOUCHED), (i, I.status, I.level)


def differ(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def run_int(c, kind, Ld, datas, period, W, H, origins, stepped=False, order="rgb", seed=0, against_full=True):
    """The integer crop: the whole buffer against the walk, then against the slices of decode_view_clips' full-size result."""
    lo, hi, dt, sgn = KINDS[kind]
    ch, cw, Cn = Ld.shape[-3:]
    n = Ld.n
    assert len(datas) == n
    buf = CG.prefill(Ld.samples, kind, seed)
    initial = [G.in_memory(w, order).copy() for w in Ld.np_windows(buf)]
    tbuf = V.to_device(c, buf)
    streams, lens = G.to_streams(c, datas)
    kw = dict(maxval=hi, stepped=stepped, order=order, signed=sgn, minval=lo if sgn else None)
    infos = c.decode_view_clips_crop(streams, lens, Ld.t_view(tbuf), period, (W, H), origins, **kw)
    windows, results = clipsx.decode(datas, initial, period, W, H, Cn, lo, hi, cw, ch, origins)
    want = buf.copy()
    for w, pic in zip(Ld.np_windows(want), windows):
        w[...] = G.in_memory(pic, order)
    got = V.to_host(tbuf, dt == np.uint16)
    differ(got, want, ("walk", kind, period, origins))
    check_infos(datas, infos, W, H, Cn)
    if against_full:
        Lf = G.dense(W, H, Cn, n)
        fbuf = CG.prefill(Lf.samples, kind, seed + 100)
        at = clipsx.expand(origins, n, period)
        for w, was, (x0, y0) in zip(Lf.np_windows(fbuf), initial, at):
            w[y0:y0 + ch, x0:x0 + cw] = G.in_memory(was, order)
        tfull = V.to_device(c, fbuf)
        infos_f = c.decode_view_clips(streams, lens, Lf.t_view(tfull), period, **dict(kw, stepped=False))
        full = Lf.np_windows(V.to_host(tfull, dt == np.uint16))
        for i, (w, (x0, y0)) in enumerate(zip(Ld.np_windows(got), at)):
            assert (w == full[i][y0:y0 + ch, x0:x0 + cw]).all(), ("slice", i, period)
        assert [CG.info_fields(I) for I in infos] == [CG.info_fields(I) for I in infos_f]
    return results


def run_float(c, kind, fkind, Ld, datas, period, W, H, origins, sets="imagenet", stepped=False, order="rgb"):
    """Float windows: the whole buffer's bits against the float walk's."""
    lo, hi = KINDS[kind][:2]
    ch, cw, Cn = Ld.shape[-3:]
    assert len(datas) == Ld.n
    scale, bias = floats.SETS[sets](hi)
    buf = floats.fill_bits(Ld.samples, fkind)
    tf, raw = floats.to_device_floats(c.device, buf, fkind)
    streams, lens = G.to_streams(c, datas)
    infos = c.decode_view_clips_crop(streams, lens, Ld.t_view(tf), period, (W, H), origins, maxval=hi, scale=scale, bias=bias, stepped=stepped,
                                     order=order, minval=lo)
    written, why = clipsx.decode_float(datas, period, W, H, Cn, lo, hi, cw, ch, origins)
    want = buf.copy()
    for w, bits in zip(Ld.np_windows(want), clipsx.float_bits(written, fkind, scale, bias, order)):
        if bits is not None:
            w[...] = bits
    differ(floats.bits_of(raw), want, ("float walk", kind, fkind, period, origins, why))
    check_infos(datas, infos, W, H, Cn)
    return why


def dest(name, cw, ch, Cn):
    return TC.DESTS[name](cw, ch, Cn)


def stack_of(cw, ch, Cn, n):
    return V.stack(cw, ch, Cn, n)


# ---- every layout, sample type and period ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TC.CASES, ids=TC._case_id)
def test_integer_crop_equals_the_walk_and_the_slice_of_the_clips_call(ctx, opts, case):
    """Every destination layout with crop-sized windows, all three sample types, gray and RGB; periods 4 and n (one clip); the
    crops, the origins and the crop route turn with the case.  The rows reach their finest level with cut residuals and a cut key
    among them: every clamp acts."""
    (W, H), Cn, name = case
    kind = TC.kind_of(case)
    k = TC.CASES.index(case)
    cw, ch = CROPS[k % 2]
    Ld, stp = dest(name, cw, ch, Cn)
    opts.set("crop_route", k % 3)
    for period in (4, Ld.n):
        datas = TC.sweep_rows(W, H, Cn, kind, Ld.n, period)
        run_int(ctx, kind, Ld, datas, period, W, H, origins_of(W, H, cw, ch, clipsx.nclips(Ld.n, period), k), stepped=stp, seed=period)


FLOAT_CASES = [c for c in TC.CASES if c[2] != "off1"]


@pytest.mark.parametrize("case", FLOAT_CASES, ids=TC._case_id)
def test_float_windows_equal_the_float_walk(ctx, opts, case):
    """float32, float16 and bfloat16 windows in every layout, over streams of uint8, 12-bit and int16 pictures, with both
    floats.SETS; crops 56x40, 33x21 and the full size."""
    (W, H), Cn, name = case
    kind = TC.kind_of(case)
    k = FLOAT_CASES.index(case)
    cw, ch = (CROPS + [(W, H)])[k % 3]
    fkind = floats.KINDS[(k // 3 + k) % 3]
    Ld, stp = dest(name, cw, ch, Cn)
    opts.set("crop_route", (k // 2) % 3)
    for period, sets in ((4, "imagenet"), (Ld.n, "identity")):
        datas = TC.sweep_rows(W, H, Cn, kind, Ld.n, period)
        org = None if (cw, ch) == (W, H) else origins_of(W, H, cw, ch, clipsx.nclips(Ld.n, period), k)
        why = run_float(ctx, kind, fkind, Ld, datas, period, W, H, org, sets, stepped=stp)
        assert set(why) <= {"key", "link"}


def test_the_float_cases_cover_every_type_and_crop():
    seen = {(floats.KINDS[(k // 3 + k) % 3], k % 3) for k in range(len(FLOAT_CASES))}
    assert len(seen) == 9
    assert {(TC.kind_of(c), c[1]) for c in FLOAT_CASES} == {(kd, Cn) for kd in KIND_NAMES for Cn in (1, 3)}


@pytest.mark.parametrize("Cn,kind,fkind", [(1, "u8", "float16"), (3, "u16", "bfloat16"), (3, "s16", "float32")])
def test_periods_1_and_5_and_thin_crops(ctx, opts, Cn, kind, fkind):
    """Periods 1 (every picture a key, an origin each) and 5; a 1-wide and a 1-high crop at the far edges."""
    W, H = 132, 72
    for period, (cw, ch) in ((1, CROPS[1]), (5, CROPS[0]), (5, THIN[0]), (4, THIN[1])):
        datas = TC.sweep_rows(W, H, Cn, kind, N, period)
        org = origins_of(W, H, cw, ch, clipsx.nclips(N, period), 1)
        run_int(ctx, kind, stack_of(cw, ch, Cn, N), datas, period, W, H, org, seed=3)
        run_float(ctx, kind, fkind, stack_of(cw, ch, Cn, N), datas, period, W, H, org)


@pytest.mark.parametrize("name", ["dense", "planar", "step"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_bgr_windows(ctx, wh, name):
    """B-G-R pixels: scale and bias belong to colours, not to memory positions."""
    W, H = wh
    kind = KIND_NAMES[(SHAPES.index(wh) + len(name)) % 3]
    fkind = floats.KINDS[(SHAPES.index(wh) + len(name)) % 3]
    cw, ch = CROPS[len(name) % 2]
    Ld, stp = dest(name, cw, ch, 3)
    datas = TC.sweep_rows(W, H, 3, kind, Ld.n, 4)
    org = origins_of(W, H, cw, ch, 3)
    run_int(ctx, kind, Ld, datas, 4, W, H, org, stepped=stp, order="bgr", seed=4)
    run_float(ctx, kind, fkind, Ld, datas, 4, W, H, org, stepped=stp, order="bgr")


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_both_crop_routes(ctx, opts, wh, route):
    W, H = wh
    opts.set("crop_route", route)
    i = SHAPES.index(wh)
    Cn, kind, fkind = (1, 3, 3)[i], KIND_NAMES[i], floats.KINDS[(i + route) % 3]
    for cw, ch in CROPS:
        datas = TC.whole_rows(W, H, Cn, kind, N, 4)
        org = origins_of(W, H, cw, ch, 3, route)
        run_int(ctx, kind, stack_of(cw, ch, Cn, N), datas, 4, W, H, org, seed=route)
        run_float(ctx, kind, fkind, stack_of(cw, ch, Cn, N), datas, 4, W, H, org)


# ---- decoder parts and the carry pictures ---------------------------------------------------------------------------------------------

SWITCHES = [("one_stream", 1), ("decode_parts", 2), ("decode_parts", 4)]


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: "%s=%d" % s)
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_whole_streams_under_the_parts(ctx, opts, wh, switch):
    """Whole streams: every part is one group of several segments.  one_stream: all segments in one launch, nothing carried.  Two
    and four parts cut clips mid-segment: a float group that starts mid-clip takes its running integers from the carry picture the
    launch before it left.  The carry cases (n = 15, period 2 and n = 11, period 3 under four parts) hold a group that reads one
    carry picture and writes the other in one launch."""
    W, H = wh
    opts.set(*switch)
    i = SHAPES.index(wh)
    for j, (n, period, _) in enumerate(CARRY + [(11, 4, 0), (11, 5, 0)]):
        Cn = (1, 3)[(i + j) % 2]
        kind, fkind = KIND_NAMES[(i + j) % 3], floats.KINDS[(i + j) % 3]
        cw, ch = CROPS[j % 2] if j != 3 else (W, H)
        datas = TC.whole_rows(W, H, Cn, kind, n, period)
        org = None if (cw, ch) == (W, H) else origins_of(W, H, cw, ch, clipsx.nclips(n, period), j)
        why = run_float(ctx, kind, fkind, stack_of(cw, ch, Cn, n), datas, period, W, H, org, sets=("imagenet", "identity")[j % 2])
        assert set(why) <= {"key", "link"}
        if (cw, ch) != (W, H):
            run_int(ctx, kind, G.dense(cw, ch, Cn, n), datas, period, W, H, org, seed=j)


def broken_rows(W, H, Cn, kind):
    """11 windows, period 4 — key, link, link cut before its finest level, link | key, link, unreadable link, link | key cut before
    its finest level, link, link.  The float walk writes windows 0, 1, 4 and 5; every part of the batch holds a window that is not
    whole, so every launch is one window and the live links 1 and 5 take their running integers from a carry picture."""
    lo, hi = KINDS[kind][:2]
    T = orc.geometry(W, H).levels
    datas = clips.streams(clips.frames(W, H, Cn, lo, hi, N), 4)
    datas[2] = levels.late_prefix(datas[2], W, H, Cn, T - 2)
    datas[6] = b"\xff\xff" + datas[6][2:]
    datas[8] = levels.late_prefix(datas[8], W, H, Cn, T - 2)
    return datas


@pytest.mark.parametrize("switch", [None] + SWITCHES[1:], ids=lambda s: "plain" if s is None else "%s=%d" % s)
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_breaks_end_a_float_clip_and_not_an_integer_one(ctx, opts, wh, switch):
    """Cut and unreadable keys and links: the integer walk goes on from what lies in memory (held to decode_view_clips' slices),
    the float walk leaves every window behind a break untouched up to the next key."""
    W, H = wh
    if switch:
        opts.set(*switch)
    i = SHAPES.index(wh)
    Cn, kind, fkind = (3, 1, 3)[i], KIND_NAMES[(i + 1) % 3], floats.KINDS[i]
    cw, ch = CROPS[i % 2]
    org = origins_of(W, H, cw, ch, 3, i)
    datas = broken_rows(W, H, Cn, kind)
    why = run_float(ctx, kind, fkind, stack_of(cw, ch, Cn, N), datas, 4, W, H, org)
    assert why == ["key", "link", "cut link", "dead", "key", "link", "unreadable link", "dead", "cut key", "dead", "dead"]
    results = run_int(ctx, kind, stack_of(cw, ch, Cn, N), datas, 4, W, H, org, seed=6)
    assert [k for k, r in enumerate(results) if r is None] == [6] and [k for k, r in enumerate(results) if r is clipsx.UNTOUCHED] == [2, 8]
    # tests/test_clips_gpu.py's mixed batch: clips 0 and 1 have no whole key, the key cut at a third is written from the planes it has
    datas = TC.mixed_rows(W, H, Cn, kind)
    why = run_float(ctx, kind, fkind, G.dense(cw, ch, Cn, N), datas, 4, W, H, org, sets="identity")
    assert why == ["cut key", "dead", "dead", "dead", "unreadable key", "dead", "dead", "dead", "key", "link", "unreadable link"]
    run_int(ctx, kind, G.dense(cw, ch, Cn, N), datas, 4, W, H, org, seed=7)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_the_clamp_fixture_behind_a_whole_key(ctx, Cn, kind):
    """Two clips of five: the four cut links of chain.clamp_fixture behind their key — whole in clip 0, clips.cut_key in clip 1:
    the floats are those of the CLAMPED integers, link after link."""
    W, H = SHAPES[KIND_NAMES.index(kind)]
    lo, hi = KINDS[kind][:2]
    key, links, _ = chain.clamp_fixture(W, H, Cn, lo, hi)
    datas = [clips.plain_stream(key)[0]] + links + [clips.cut_key(W, H, Cn, lo, hi)[0]] + links
    cw, ch = CROPS[Cn // 3]
    org = origins_of(W, H, cw, ch, 2, Cn)
    fkind = floats.KINDS[(KIND_NAMES.index(kind) + Cn) % 3]
    assert run_float(ctx, kind, fkind, stack_of(cw, ch, Cn, 10), datas, 5, W, H, org) == ["key"] + ["link"] * 4 + ["key"] + ["link"] * 4
    results = run_int(ctx, kind, G.dense(cw, ch, Cn, 10), datas, 5, W, H, org, seed=8)
    assert any((a != b).any() for a, b in zip(results[1:5], results[6:]))


# ---- the identity ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn,kind", [(1, "u16"), (3, "u8"), (3, "s16")])
def test_a_full_size_crop_without_a_format_is_the_clips_call(ctx, Cn, kind):
    import torch

    W, H = 263, 135
    lo, hi, dt, sgn = KINDS[kind]
    datas = TC.mixed_rows(W, H, Cn, kind)
    streams, lens = G.to_streams(ctx, datas)
    Ld = V.stack(W, H, Cn, N)
    kw = dict(maxval=hi, signed=sgn, minval=lo if sgn else None)
    a = TC.Run(ctx, kind, Ld, seed=9)
    infos_a = a.clips(streams, lens, 4)
    for origins in (None, (0, 0), [(0, 0)] * 3):
        b = TC.Run(ctx, kind, Ld, seed=9)
        infos_b = ctx.decode_view_clips_crop(streams, lens, Ld.t_view(b.tbuf), 4, (W, H), origins, **kw)
        assert torch.equal(a.tbuf, b.tbuf)
        assert [CG.info_fields(I) for I in infos_a] == [CG.info_fields(I) for I in infos_b]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_with_their_texts_and_nothing_written(ctx):
    import torch

    import dwt_amd

    W, H, n, cw, ch = 132, 72, 4, 56, 40
    t = torch.full((n, ch, cw, 1), 7, dtype=torch.uint8, device=ctx.device)
    f = torch.full((n, ch, cw, 1), 7.0, dtype=torch.float16, device=ctx.device)
    streams = torch.zeros((n, 4096), dtype=torch.uint8, device=ctx.device)
    lens = torch.full((n,), 100, dtype=torch.int64, device=ctx.device)

    def refused(start, into, *args, **kw):
        with pytest.raises(dwt_amd.DwtxError) as e:
            ctx.decode_view_clips_crop(streams, lens, into, *args, **kw)
        text = str(e.value)
        assert e.value.rc == ERR_ARG and "clips view:" in text and start in text, text

    refused("clips view: origin (77, 0) of clip 1", t, 2, (W, H), [(0, 0), (W - cw + 1, 0)])
    refused("clips view: origin (0, -1) of clip 0", f, 2, (W, H), [(0, -1), (0, 0)], scale=2.0)
    refused("clips view: crop 56x40", t, 2, (48, 72))
    refused("clips view: crop 56x40", f, 2, (132, 32))
    refused("clips view: unsupported image size", t, 2, (4, 4))
    refused("clips view: maxval 100", t, 2, (W, H), maxval=100)
    refused("minval < maxval", f, 2, (W, H), minval=50, maxval=10)
    refused("clips view: windows overlap", t.as_strided((n, ch, cw, 1), (cw * ch - cw, cw, 1, 1)), 2, (W, H))
    lib, Cc = ctx.lib, dwt_amd.C
    infos = (dwt_amd.DecodeInfo * n)()
    v = ctx._view(f, 255, floats=True)[0]

    def c_call(view, fmt, period=2):
        return lib.dwtx_decode_view_clips_crop(ctx.h, streams.data_ptr(), streams.shape[1], lens.data_ptr(), W, H, n, view, 0, period, 0, 0, 0,
                                               fmt, cw, ch, None, Cc.cast(infos, Cc.c_void_p))

    def text():
        return lib.dwtx_last_error().decode()

    bad = dwt_amd.float_format("float16")
    bad.type = 5
    assert c_call(Cc.byref(v), Cc.byref(bad)) == ERR_ARG and text().startswith("clips view: float type 5"), text()
    assert c_call(Cc.byref(v), Cc.byref(dwt_amd.float_format("float32"))) == ERR_ARG and text().startswith("clips view: sample_bytes 2 does not match"), text()
    bad = dwt_amd.float_format("float16")
    bad.bias[1] = float("inf")
    assert c_call(Cc.byref(v), Cc.byref(bad)) == ERR_ARG and text().startswith("clips view: scale[1]") and "finite" in text(), text()
    assert c_call(Cc.byref(v), Cc.byref(dwt_amd.float_format("float16")), period=0) == ERR_ARG and text().startswith("clips view: period 0"), text()
    assert c_call(None, None) == ERR_ARG and text().startswith("clips view: no view"), text()
    assert (t == 7).all() and (f == 7).all()
    # in Python, before any device call
    wrong = [dict(flip="y"), dict(levels_max=2), dict(key=t[0]), dict(windows=[t[0]]), dict(base=t), dict(origins=[(0, 0)] * n), dict(origins=[(0, 0)] * 3),
             dict(scale=2.0), dict(bias=(1.0, 2.0, 3.0))]
    for kw in wrong:
        with pytest.raises(ValueError):
            ctx.decode_view_clips_crop(streams, lens, t, 2, (W, H), **kw)
    for period in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError):
            ctx.decode_view_clips_crop(streams, lens, f, period, (W, H))
    with pytest.raises(ValueError):
        ctx.decode_view_clips_crop(streams, lens, [t[0], t[1]], 2, (W, H))
    with pytest.raises(ValueError):
        ctx.decode_view_clips_crop(streams, lens, f, 2, (W, H), scale=(1.0, 2.0))
    with pytest.raises(ValueError):
        ctx.decode_view_clips_crop(streams, lens, f, 2, (W, H), signed=True)
    # decode_view_clips keeps its refusals
    for kw in (dict(crop=(cw, ch)), dict(origins=[(0, 0)]), dict(scale=1.0)):
        with pytest.raises(ValueError):
            ctx.decode_view_clips(streams, lens, t, 2, **kw)
    with pytest.raises(ValueError):
        ctx.decode_view_clips(streams, lens, f, 2)
    assert (t == 7).all() and (f == 7).all()


# ---- the context's history ----------------------------------------------------------------------------------------------------------

@pytest.fixture
def fresh(ctx):
    """A context that has run nothing yet (it depends on `ctx`: no GPU, no test)"""
    import dwt_amd

    c = dwt_amd.Context(0)
    yield c
    c.close()


def test_a_float_call_as_a_contexts_first_call(fresh):
    """The carry pictures and the crop's table are asked for by a context that has no scratch at all."""
    W, H, Cn, kind = 263, 135, 3, "u8"
    fresh.set_option("decode_parts", 4)
    n, period, _ = CARRY[0]
    cw, ch = CROPS[1]
    datas = TC.whole_rows(W, H, Cn, kind, n, period)
    run_float(fresh, kind, "float16", stack_of(cw, ch, Cn, n), datas, period, W, H, origins_of(W, H, cw, ch, clipsx.nclips(n, period)))


@pytest.mark.parametrize("Cn,kind,fkind", [(1, "s16", "bfloat16"), (3, "u8", "float32")], ids=["gray-s16", "rgb-u8"])
def test_a_call_after_calls_of_another_geometry_channel_count_and_depth(fresh, Cn, kind, fkind):
    """tests/history.py's dirt on a private context — the other channel count, a transposed geometry, 16-bit depth, a larger float
    call that leaves carry pictures behind — then the broken batch, whole results compared."""
    W, H = 263, 135
    datas = broken_rows(W, H, Cn, kind)
    stride = history.stride_of(datas)
    for cl in (history.call("decode", W, H, 3, n=12, stride=stride), history.call("decode16", H + 1, W + 1, 4 - Cn, n=12, stride=stride),
               history.call("decode", W, H, Cn, n=12, stride=stride)):
        history.dirty(fresh, cl.W, cl.H, cl.Cn, cl.n, cl.how, cl.kind, cl.stride)
    fresh.set_option("decode_parts", 4)
    run_float(fresh, kind, fkind, stack_of(W, H, Cn, N), TC.whole_rows(W, H, Cn, kind, N, 3), 3, W, H, None, sets="identity")
    cw, ch = CROPS[0]
    org = origins_of(W, H, cw, ch, 3)
    run_float(fresh, kind, fkind, stack_of(cw, ch, Cn, N), datas, 4, W, H, org)
    run_int(fresh, kind, stack_of(cw, ch, Cn, N), datas, 4, W, H, org, seed=12)
