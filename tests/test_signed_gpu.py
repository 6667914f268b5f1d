"""GPU: signed 16-bit samples — dwtx_encode_view_signed / dwtx_decode_view_signed and the host pair dwtx_encode_images_s16 /
dwtx_decode_images_s16 (include/dwtx.h): int16 pictures coded as the integers they hold.

The yardstick is the oracle on the CPU (tests/signed.py over tests/deep.py): deep_encode's bytes and counters for every
encode, signed_decode's samples for every decode.  Every comparison is exact and covers the WHOLE buffer: a stream buffer
is prefilled and must hold the oracle's bytes, the zero padding the contract names and the fill behind it; a destination
holds the oracle's picture in each window's corner and its fill pattern — negative values among it — in every other sample.
Layouts are flat buffers of samples plus an offset, a shape and strides, as in tests/test_views_gpu.py; n is 3 to 5."""
import ctypes as C

import numpy as np
import pytest

import deep
import orc
import signed
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
# 132x72 and 520x264: W % 4 == 0 and more than 64 on a side — views on the quad grid are read and written by the transform's finest
# level itself (the deep sources' signed twins, the deep and float sinks with the lower clamp; one and two wide levels), views off it
# and everything under DWTX_OPT_NO_PIXELS16 by the general conversions; 263x135: W % 4 != 0, the general conversions always
SHAPES = signed.SHAPES
RANGES = signed.RANGES
FILL = 0xA5


# ---- layouts: (Layout, stepped) by name; all strides in samples -------------------------------------------------------------------

def dense(W, H, Cn, n=3):
    return V.Layout(n * H * W * Cn, 0, (n, H, W, Cn), (H * W * Cn, W * Cn, Cn, 1))


def nchw(W, H, n=3, off=8):
    img = 3 * H * W + 12
    return V.Layout(off + n * img + 5, off, (n, H, W, 3), (img, W, 1, H * W + 4))


def stepped(W, H, Cn, step, n=3):
    pitch = W * step + 4
    return V.Layout(4 + n * H * pitch, 4, (n, H, W, Cn), (H * pitch, pitch, step, 1))


LAYOUTS = {
    "dense": lambda W, H, Cn: (dense(W, H, Cn), False),
    "grid": lambda W, H, Cn: (V.grid(W, H, Cn, "quad", rows=2, cols=2), False),           # pitched windows on the quad
    "grid-off1": lambda W, H, Cn: (V.grid(W, H, Cn, "off1", rows=2, cols=2), False),      # one column off it
    "grid-pitch": lambda W, H, Cn: (V.grid(W, H, Cn, "pitch", rows=2, cols=2), False),    # a pitch that is no multiple of 4
    "stack": lambda W, H, Cn: (V.stack(W, H, Cn), False),
    "nchw": lambda W, H, Cn: (nchw(W, H), False),                                         # (RGB only: LAYOUT_CASES)
    "step": lambda W, H, Cn: (stepped(W, H, Cn, 4 if Cn == 3 else 2), True),              # RGBX-style step 4, gray step 2
}


LAYOUT_CASES = [(wh, Cn, layout) for wh in SHAPES for Cn in (1, 3) for layout in LAYOUTS if Cn == 3 or layout != "nchw"]
_case_id = lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], "gray" if c[1] == 1 else "rgb", c[2])   # noqa: E731


def fill16(samples):
    """A buffer's fill: every int16 value class, negative ones among them."""
    i = np.arange(samples, dtype=np.int64)
    return ((i * 7919 + (i >> 7) * 13) % 65521 - 32760).astype(np.int16)


def in_memory(pic, order, flip):
    """A picture [h, w, C] as it lies in its window: B, G, R under order="bgr"; mirrored under the flip flags (x = 1, y = 2)."""
    m = pic[..., ::-1] if order == "bgr" else pic
    if flip & 1:
        m = m[:, ::-1]
    if flip & 2:
        m = m[::-1]
    return m


def flags_of(flip, n):
    if flip is None:
        return [0] * n
    if isinstance(flip, (list, tuple)):
        return [{"": 0, "x": 1, "y": 2, "xy": 3}.get(f, f) for f in flip]
    return [{"x": 1, "y": 2, "xy": 3}[flip]] * n


_oracle = {}


def oracle_encode(pic, capacity=0):
    key = (pic.tobytes(), pic.shape, capacity)
    if key not in _oracle:
        _oracle[key] = deep.deep_encode(pic, capacity)
    return _oracle[key]


def pictures(W, H, Cn, lo, hi, n):
    """n different pictures of a range: smooth + noise, blocks, noise, smooth + noise ..."""
    kinds = ["smooth_noise", "blocks", "noise", "smooth_noise", "smooth_noise"]
    return [signed.stream(kinds[i], W, H, Cn, lo, hi, 3 if kinds[i] == "blocks" else i + 1)[0] for i in range(n)]


# ---- encode ------------------------------------------------------------------------------------------------------------------------

def check_streams(out, info, pics, capacity=0, refused=()):
    """The whole stream buffer (prefilled with FILL) and the records against the oracle."""
    host = out.cpu().numpy()
    infos = V.infos_of(info)
    stride = host.shape[1]
    for i, pic in enumerate(pics):
        I = infos[i]
        if i in refused:
            assert I.error == 1, i
            continue
        want, st = oracle_encode(pic, capacity)
        Cn = pic.shape[2]
        assert I.error == 0 and I.nbytes == len(want), (i, I.error, I.nbytes, len(want))
        assert host[i, :I.nbytes].tobytes() == want, i
        assert list(I.planes)[:Cn] == list(st.planes)[:Cn] and (I.root_bits, I.total_bits) == (st.root_bits, st.total_bits), i
        if capacity <= 0:   # (the zero padding after a stream that CAPACITY does not cut, and the slot's bytes beyond left as they were)
            pad = min(stride, (I.nbytes + 3) // 4 * 4 + 16)
            assert not host[i, I.nbytes:pad].any(), i
            assert (host[i, pad:] == FILL).all(), i


def check_encode(ctx, L, pics, stepped=False, order="rgb", flip=None, listed=None, capacities=(0, 500)):
    """pics[i] is window i's picture; listed: a permutation — the windows go as a list in that order."""
    import torch

    H, W, Cn = pics[0].shape
    buf = fill16(L.samples)
    fl = flags_of(flip, L.n)
    for w, p, f in zip(L.np_windows(buf), pics, fl):
        w[...] = in_memory(p, order, f)
    tbuf = torch.from_numpy(buf.copy()).to(ctx.device)
    tv = L.t_view(tbuf)
    stride = ctx.lib.dwtx_encode_bound16(W, H, Cn)
    for capacity in capacities:
        out = torch.full((L.n if listed is None else len(listed), stride if capacity <= 0 else (capacity + 15) // 8 * 8), FILL, dtype=torch.uint8, device=ctx.device)
        if listed is None:
            out, info = ctx.encode_view(tv, capacity, out=out, stepped=stepped, order=order, flip=flip, signed=True)
            check_streams(out, info, pics, capacity)
        else:
            wins = [tv[i] if tv.dim() == 4 else tv[i // tv.shape[1], i % tv.shape[1]] for i in listed]
            out, info = ctx.encode_view_list(wins, capacity=capacity, out=out, stepped=stepped, order=order,
                                             flip=None if flip is None else [fl[i] for i in listed], signed=True)
            check_streams(out, info, [pics[i] for i in listed], capacity)
    assert (tbuf.cpu().numpy() == buf).all(), "the source was written to"


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_case_id)
def test_signed_encode_equals_the_oracle(ctx, case):
    (W, H), Cn, layout = case
    L, stp = LAYOUTS[layout](W, H, Cn)
    lo, hi = RANGES[(W + Cn) % 2]
    check_encode(ctx, L, pictures(W, H, Cn, lo, hi, L.n), stepped=stp)


@pytest.mark.parametrize("layout", ["dense", "nchw", "step"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_encode_of_bgr_pixels(ctx, wh, layout):
    W, H = wh
    L, stp = LAYOUTS[layout](W, H, 3)
    check_encode(ctx, L, pictures(W, H, 3, -2048, 2047, L.n), stepped=stp, order="bgr", capacities=(0,))


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_encode_of_a_scattered_list(ctx, wh, Cn):
    W, H = wh
    L = V.grid(W, H, Cn, "quad", rows=2, cols=2)
    check_encode(ctx, L, pictures(W, H, Cn, -1024, 3071, 4), listed=[2, 0, 3, 0, 1], capacities=(0,))


@pytest.mark.parametrize("flip", ["y", "x", ["", "x", "y", "xy"]], ids=["y", "x", "each"])
@pytest.mark.parametrize("layout", ["grid", "nchw", "step"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_encode_of_flipped_windows(ctx, wh, layout, flip):
    W, H = wh
    for Cn in (1, 3) if layout != "nchw" else (3,):
        L, stp = LAYOUTS[layout](W, H, Cn)
        f = flip[:L.n] if isinstance(flip, list) else flip
        check_encode(ctx, L, pictures(W, H, Cn, -2048, 2047, L.n), stepped=stp, flip=f, capacities=(0,))


@pytest.mark.parametrize("option", ["no_pixels16", "no_square_tiles", "exact_orders"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_encode_under_the_switches(ctx, opts, wh, option):
    """Each switch on (off: every other test): paths that must agree.  no_pixels16 sends the views on the quad grid, which the
    wide signed sources read otherwise, through the general conversion."""
    W, H = wh
    opts.set(option, 1)
    for Cn in (1, 3):
        L = V.grid(W, H, Cn, "quad", rows=2, cols=2)
        check_encode(ctx, L, pictures(W, H, Cn, -1024, 3071, L.n), capacities=(0,))
    check_encode(ctx, nchw(W, H), pictures(W, H, 3, -2048, 2047, 3), order="bgr", flip="y", capacities=(0,))


@pytest.mark.parametrize("rows_per_wave", [4, 16, 64])
@pytest.mark.parametrize("wh", [(132, 72), (520, 264), (260, 131)], ids=lambda wh: "%dx%d" % wh)
def test_signed_wide_kernels_at_the_strip_edges(ctx, opts, wh, rows_per_wave):
    """The wide signed sources and sinks under every strip height, at a width one lane into a second strip (260) and a last row
    pair without its odd row (131): encode and decode, gray, interleaved, planar and B, G, R, with and without NO_PIXELS16 —
    the two routes of one view give the oracle's bytes and samples."""
    W, H = wh
    opts.set("lift_rows", rows_per_wave)
    lo, hi = -2048, 2047
    for no16 in (0, 1):
        opts.set("no_pixels16", no16)
        for Cn, L, order in ((1, V.grid(W, H, 1, "quad", rows=2, cols=2), "rgb"), (3, dense(W, H, 3, 4), "bgr"), (3, nchw(W, H, 4), "rgb")):
            check_encode(ctx, L, pictures(W, H, Cn, lo, hi, 4), order=order, capacities=(0,))
            check_decode(ctx, L, W, H, Cn, decode_rows(W, H, Cn, lo, hi, 4), lo, hi, order=order)
            check_decode(ctx, L, W, H, Cn, decode_rows(W, H, Cn, lo, hi, 4), lo, hi, order=order, flip=["xy", "y", "x", ""])


def test_full_range_noise_is_refused_alone(ctx):
    """Uniform int16 noise over the full range needs 17 planes: refused, while its neighbours' streams are the oracle's."""
    W, H = 132, 72
    pics = pictures(W, H, 1, -1024, 3071, 3)
    pics[1] = signed.noise(W, H, 1, -32768, 32767, 4)
    assert list(oracle_encode(pics[1])[1].planes)[:1] == [17]
    import torch

    t = torch.from_numpy(np.stack(pics)).to(ctx.device)
    out = torch.full((3, ctx.lib.dwtx_encode_bound16(W, H, 1)), FILL, dtype=torch.uint8, device=ctx.device)
    out, info = ctx.encode_view(t, out=out, signed=True)
    check_streams(out, info, pics, refused={1})


def test_a_zero_crossing_picture_with_and_without_the_keyword(ctx):
    """signed=True: the oracle's bytes of the signed integers.  Without the keyword an int16 tensor is what it has always
    been, the carrier of uint16 bytes: the uint16 reading's result — here its refusal (17 planes)."""
    import torch

    W, H = 132, 72
    pics = [signed.zero_crossing(W, H, 1), signed.zero_crossing(W, H, 1)[::-1].copy()]
    t = torch.from_numpy(np.stack(pics)).to(ctx.device)
    out = torch.full((2, ctx.lib.dwtx_encode_bound16(W, H, 1)), FILL, dtype=torch.uint8, device=ctx.device)
    out, info = ctx.encode_view(t, out=out, signed=True)
    check_streams(out, info, pics)
    assert V.infos_of(info)[0].planes[0] == 7
    out, info = ctx.encode_view(t)
    for i, I in enumerate(V.infos_of(info)):
        st = deep.deep_encode(pics[i].view(np.uint16))[1]
        assert st.planes[0] == 17 and I.error == 1 and I.planes[0] == 17


# ---- decode ------------------------------------------------------------------------------------------------------------------------

def to_streams(ctx, rows):
    import torch

    stride = (max(len(r) for r in rows) + 64 + 7) // 8 * 8
    host = np.full((len(rows), stride), FILL, dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return torch.from_numpy(host).to(ctx.device), torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)


def place(w, ref, order, flip, origin=(0, 0)):
    """The oracle's picture `ref` (or, with an origin, the part of it from there on) into window w, as memory holds it."""
    x0, y0 = origin
    part = ref[y0:y0 + w.shape[0], x0:x0 + w.shape[1]]
    if part.size == 0:
        return
    m = w
    if flip & 2:
        m = m[::-1]
    if flip & 1:
        m = m[:, ::-1]
    m[:part.shape[0], :part.shape[1]] = part[..., ::-1] if order == "bgr" else part


def check_decode(ctx, L, W, H, Cn, rows, lo, hi, levels_max=-1, stepped=False, order="rgb", flip=None, listed=False, crop=None, origins=None,
                 dtype=None, scale=1.0, bias=0.0):
    """rows: one stream per window.  dtype None: int16 windows; else a torch float type, with scale and bias.  crop: (cw, ch), the
    windows' size (L is then a layout of cw x ch windows).  The whole buffer afterwards."""
    import torch

    n = L.n
    g = orc.geometry(W, H)
    pixels_max = -1 if levels_max < 0 else g.pixels[levels_max]
    fl = flags_of(flip, n)
    refs = [signed.signed_decode(r, W, H, Cn, lo, hi, pixels_max) for r in rows]
    if dtype is None:
        buf = fill16(L.samples)
        want = buf.copy()
        for i, (w, ref) in enumerate(zip(L.np_windows(want), refs)):
            if ref is not None:
                place(w, ref, order, fl[i], origins[i] if origins else (0, 0))
        tbuf = torch.from_numpy(buf.copy()).to(ctx.device)
    else:
        fbuf = (torch.from_numpy(fill16(L.samples).astype(np.float32)) * 0.37).to(dtype)
        wantt = fbuf.clone()
        s3 = torch.tensor(np.broadcast_to(np.asarray(scale, dtype=np.float32), (3,)).copy())[:Cn]
        b3 = torch.tensor(np.broadcast_to(np.asarray(bias, dtype=np.float32), (3,)).copy())[:Cn]
        view = L.t_view(wantt)
        wins = [view[i] if view.dim() == 4 else view[i // view.shape[1], i % view.shape[1]] for i in range(n)]
        for i, (w, ref) in enumerate(zip(wins, refs)):
            if ref is None:
                continue
            x0, y0 = origins[i] if origins else (0, 0)
            part = ref[y0:y0 + w.shape[0], x0:x0 + w.shape[1]]
            if part.size == 0:
                continue
            val = ((torch.from_numpy(part.astype(np.float32)) * s3) + b3).to(dtype)   # two float32 roundings, then the type
            if order == "bgr":
                val = val.flip(-1)
            ph, pw = part.shape[:2]
            ys, xs = slice(0, ph), slice(0, pw)
            if fl[i] & 2:   # (torch's flip copies: the mirrored corner is addressed, the values are mirrored)
                val, ys = val.flip(0), slice(w.shape[0] - ph, w.shape[0])
            if fl[i] & 1:
                val, xs = val.flip(1), slice(w.shape[1] - pw, w.shape[1])
            w[ys, xs] = val
        tbuf = fbuf.clone().to(ctx.device)
    streams, lens = to_streams(ctx, rows)
    tv = L.t_view(tbuf)
    kw = dict(maxval=hi, minval=lo, levels_max=levels_max, stepped=stepped, order=order, flip=flip)
    if dtype is None:
        kw["signed"] = True
    else:
        kw.update(scale=scale, bias=bias)
    if listed:
        wins = [tv[i] if tv.dim() == 4 else tv[i // tv.shape[1], i % tv.shape[1]] for i in range(n)]
        infos = ctx.decode_view_list(streams, lens, wins, size=(W, H) if crop else None, origins=origins, **kw)
    elif crop:
        infos = ctx.decode_view_crop(streams, lens, tv, (W, H), origins=origins, **kw)
    elif dtype is None:
        infos = ctx.decode_view(streams, lens, tv, **kw)
    else:
        infos = ctx.decode_view_float(streams, lens, tv, **kw)
    if dtype is None:
        got = tbuf.cpu().numpy()
        bad = np.flatnonzero(got != want)
    else:
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        bad = np.flatnonzero((tbuf.cpu().view(bits) != wantt.view(bits)).numpy())
    assert bad.size == 0, f"{bad.size} samples differ, first at {bad[:5]} of {L.samples} (view offset {L.off}, strides {L.strides})"
    for I, r, ref in zip(infos, rows, refs):
        assert (I.status != 0) == (ref is None)
        if ref is not None:
            assert I.level == deep.decoded(r, W, H, Cn, pixels_max)[0]
    return infos


def decode_rows(W, H, Cn, lo, hi, n):
    """n streams of a range: whole ones and the two clamp fixtures (tests/test_signed_cpu.py holds those to their condition)."""
    whole = [signed.stream(k, W, H, Cn, lo, hi, s)[1] for k, s in (("smooth_noise", 1), ("blocks", 3), ("smooth_noise", 2))]
    rows = [whole[0], signed.cut_fixture(W, H, Cn, lo, hi, 0.33), whole[1], signed.cut_fixture(W, H, Cn, lo, hi, 0.6), whole[2]]
    return rows[:n]


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_case_id)
def test_signed_decode_equals_the_oracle(ctx, case):
    """Whole streams and the cut fixtures, on which every clamp of the range acts, into every sink."""
    (W, H), Cn, layout = case
    L, stp = LAYOUTS[layout](W, H, Cn)
    for lo, hi in RANGES:
        check_decode(ctx, L, W, H, Cn, decode_rows(W, H, Cn, lo, hi, L.n), lo, hi, stepped=stp)


@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_decode_bgr_lists_and_flips(ctx, wh):
    W, H = wh
    lo, hi = -2048, 2047
    rows = decode_rows(W, H, 3, lo, hi, 4)
    check_decode(ctx, dense(W, H, 3, 4), W, H, 3, rows, lo, hi, order="bgr")
    L, stp = LAYOUTS["step"](W, H, 3)
    check_decode(ctx, L, W, H, 3, rows[:L.n], lo, hi, stepped=stp, order="bgr")
    for Cn in (1, 3):
        L = V.grid(W, H, Cn, "quad", rows=2, cols=2)
        r = decode_rows(W, H, Cn, lo, hi, 4)
        check_decode(ctx, L, W, H, Cn, r, lo, hi, listed=True)
        for flip in ("y", "x", ["", "x", "y", "xy"]):
            check_decode(ctx, L, W, H, Cn, r, lo, hi, flip=flip)
    check_decode(ctx, nchw(W, H, 4), W, H, 3, rows, lo, hi, flip=["xy", "y", "x", ""])


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_decode_at_every_level(ctx, wh, Cn):
    """Reduced pictures lie in their windows' corners — under a flip in the corner where their pixel (0, 0) lies."""
    W, H = wh
    lo, hi = -1024, 3071
    L = V.grid(W, H, Cn, "quad", rows=2, cols=2)
    rows = decode_rows(W, H, Cn, lo, hi, 4)
    for lm in range(orc.geometry(W, H).levels + 1):
        check_decode(ctx, L, W, H, Cn, rows, lo, hi, levels_max=lm)
    if W % 4 == 0:   # (a mirrored window wider than its reduced picture needs its width on the quad)
        check_decode(ctx, L, W, H, Cn, rows, lo, hi, levels_max=2, flip=["xy", "y", "x", ""])


@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_decode_batches_parts_and_an_unreadable_stream(ctx, opts, wh):
    W, H = wh
    lo, hi = -2048, 2047
    for Cn in (1, 3):
        rows = decode_rows(W, H, Cn, lo, hi, 5)
        rows[2] = rows[2][:5]   # unreadable: status 1, its window untouched
        L = dense(W, H, Cn, 5)
        for name, value in (("decode_parts", 2), ("decode_parts", 4), ("one_stream", 1)):
            opts.set(name, value)
            infos = check_decode(ctx, L, W, H, Cn, rows, lo, hi)
            assert [I.status for I in infos] == [0, 0, 1, 0, 0]
            opts.set(name, 0)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_decode_into_floats(ctx, wh, dtype):
    """A CT slice straight into Hounsfield units: scale and bias on the signed, clamped integers."""
    import torch

    W, H = wh
    dt = getattr(torch, dtype)
    lo, hi = -1024, 3071
    for Cn, layout, scale, bias in ((1, "grid", 0.25, -3.5), (3, "nchw", [1 / 1024, 1 / 512, 1 / 2048], [0.5, -0.25, 1.0]),
                                    (3, "dense", 1.0, 0.0), (1, "step", 1 / 3, 7.0)):
        L, stp = LAYOUTS[layout](W, H, Cn)
        check_decode(ctx, L, W, H, Cn, decode_rows(W, H, Cn, lo, hi, L.n), lo, hi, stepped=stp, dtype=dt, scale=scale, bias=bias)


@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_signed_crops(ctx, opts, wh, route):
    import torch

    W, H = wh
    lo, hi = -2048, 2047
    opts.set("crop_route", route)
    cw, ch = 50, 33
    origins = [(0, 0), (W - cw, H - ch), (17, 5), (W // 2, 1)]
    for Cn in (1, 3):
        rows = decode_rows(W, H, Cn, lo, hi, 4)
        L = V.grid(cw, ch, Cn, "quad", rows=2, cols=2)
        check_decode(ctx, L, W, H, Cn, rows, lo, hi, crop=(cw, ch), origins=origins)
        check_decode(ctx, L, W, H, Cn, rows, lo, hi, crop=(cw, ch), origins=origins, flip=["x", "", "xy", "y"], listed=True)
    check_decode(ctx, nchw(cw, ch, 4), W, H, 3, decode_rows(W, H, 3, lo, hi, 4), lo, hi, crop=(cw, ch), origins=origins, dtype=torch.float16,
                 scale=0.5, bias=-1.0)


# ---- float sources -----------------------------------------------------------------------------------------------------------------

def float_source(W, H, Cn, lo, hi, kind, scale, bias, seed):
    """float samples [H, W, Cn] of type `kind` (a torch tensor) whose quantised picture is smooth + noise over more than the
    range, with planted NaNs, infinities, -0.0 and ties, and that picture (signed.quantise of the very bits)."""
    import torch

    rng = np.random.default_rng(seed)
    span = hi - lo
    target = deep.smooth_noise(W, H, Cn, span + span // 4, seed).astype(np.float64) + lo - span // 8   # both clamps act
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64), (Cn,))
    b = np.broadcast_to(np.asarray(bias, dtype=np.float64), (Cn,))
    x = (target + rng.uniform(-0.5, 0.5, target.shape) - b) / s
    flat = x.reshape(-1)
    flat[rng.choice(flat.size, 24, replace=False)] = np.tile([np.nan, np.inf, -np.inf, -0.0, 0.5, -0.5, 1.5, -2.5], 3)
    t = torch.from_numpy(x.astype(np.float32)).to(getattr(torch, kind))
    return t, signed.quantise(t.float().numpy(), scale, bias, lo, hi).astype(np.int16)


@pytest.mark.parametrize("rng", [(-100, 155), (-1024, 3071), (5, 100)], ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("kind", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_float_sources_with_a_lower_bound(ctx, wh, kind, rng):
    """maxval <= 255 and above, minval below 0 (and one above it): the oracle's encode of signed.quantise of the floats."""
    import torch

    W, H = wh
    lo, hi = rng
    for Cn, layout, scale, bias in ((1, "grid", 4.0, -0.25), (3, "nchw", [2.0, 0.5, 8.0], [0.0, 1.5, -3.0]), (3, "dense", 1.0, 0.0)):
        L, stp = LAYOUTS[layout](W, H, Cn)
        made = [float_source(W, H, Cn, lo, hi, kind, scale, bias, i + 1) for i in range(L.n)]
        pics = [m[1] for m in made]
        assert all(p.min() == lo and p.max() == hi for p in pics)
        fbuf = (torch.from_numpy(fill16(L.samples).astype(np.float32)) * 0.37).to(getattr(torch, kind))
        fbuf[::97] = float("nan")
        view = L.t_view(fbuf)
        for i, m in enumerate(made):
            (view[i] if view.dim() == 4 else view[i // view.shape[1], i % view.shape[1]])[...] = m[0]
        tv = L.t_view(fbuf.to(ctx.device))
        out = torch.full((L.n, ctx.lib.dwtx_encode_bound16(W, H, Cn)), FILL, dtype=torch.uint8, device=ctx.device)
        out, info = ctx.encode_view_float(tv, maxval=hi, minval=lo, scale=scale, bias=bias, out=out, stepped=stp)
        check_streams(out, info, pics)
        if Cn == 1:
            out.fill_(FILL)
            out, info = ctx.encode_view_float(tv, maxval=hi, minval=lo, scale=scale, bias=bias, out=out, flip="x")
            check_streams(out, info, [p[:, ::-1].copy() for p in pics])


# ---- the three equivalences --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_equivalences_with_the_unsigned_calls(ctx, wh, Cn):
    import torch

    W, H = wh
    M = 4095
    L = V.grid(W, H, Cn, "quad", rows=2, cols=2)
    pics = [deep.smooth_noise(W, H, Cn, M, i + 1) for i in range(L.n)]
    buf = fill16(L.samples)
    for w, p in zip(L.np_windows(buf), pics):
        w[...] = p.astype(np.int16)
    tv = L.t_view(torch.from_numpy(buf).to(ctx.device))
    # 1. integer samples all in [0, 32767]: the bytes and records of the unsigned call
    so, si = ctx.encode_view(tv, signed=True)
    uo, ui = ctx.encode_view(tv)
    assert [V.fields(a) for a in V.infos_of(si)] == [V.fields(a) for a in V.infos_of(ui)]
    for i, I in enumerate(V.infos_of(si)):   # (the slots' bytes behind a stream and its padding are whatever they were)
        assert I.error == 0 and (so[i, :I.nbytes] == uo[i, :I.nbytes]).all()
        assert so[i, :I.nbytes].cpu().numpy().tobytes() == deep.deep_encode(pics[i])[0]
    # 2. minval == 0: the decode gives the unsigned call's samples bit for bit, on streams the clamps act on
    rows = [deep.deep_encode(deep.blocks(W, H, Cn, M, 3))[0]] * L.n
    rows = [rows[0], rows[0][:len(rows[0]) // 3], rows[0][:len(rows[0]) * 3 // 5], rows[0][:len(rows[0]) // 2]]
    streams, lens = to_streams(ctx, rows)
    a, b = torch.from_numpy(fill16(L.samples)).to(ctx.device), torch.from_numpy(fill16(L.samples)).to(ctx.device)
    ctx.decode_view(streams, lens, L.t_view(a), maxval=M, minval=0, signed=True)
    ctx.decode_view(streams, lens, L.t_view(b), maxval=M)
    assert (a == b).all()
    want = fill16(L.samples)
    for w, r in zip(L.np_windows(want), rows):
        ref = deep.deep_decode(r, W, H, Cn, M)
        w[:ref.shape[0], :ref.shape[1]] = ref.astype(np.int16)
    assert (a.cpu().numpy() == want).all()
    # 3. fmt given and minval == 0: the call is the flip call (here through the library's own entry point)
    import dwt_amd

    fa, fb = [torch.full((L.samples,), -7.0, dtype=torch.float16, device=ctx.device) for _ in range(2)]
    fmt = dwt_amd.float_format(torch.float16, 0.5, 1.0)
    for t, sym, extra in ((fa, "dwtx_decode_view_signed", (0,)), (fb, "dwtx_decode_view_flip", ())):
        v = ctx._view(L.t_view(t), M, floats=True)[0]
        infos = (dwt_amd.DecodeInfo * L.n)()
        rc = getattr(ctx.lib, sym)(ctx.h, streams.data_ptr(), streams.shape[1], lens.data_ptr(), W, H, L.n, -1, C.byref(v), 0, 0, C.byref(fmt), W, H,
                                   None, None, 2, None, *extra, C.cast(infos, C.c_void_p))
        assert rc == 0
    assert (fa.view(torch.int16) == fb.view(torch.int16)).all() and (fa != -7.0).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_every_refusal_has_a_text_and_writes_nothing(ctx):
    import torch

    import dwt_amd

    W, H, n = 132, 72, 3
    lib = ctx.lib
    pics = pictures(W, H, 1, -1024, 3071, n)
    rows = [oracle_encode(p)[0] for p in pics]
    streams, lens = to_streams(ctx, rows)
    src = torch.from_numpy(np.stack(pics)).to(ctx.device)
    dst = torch.from_numpy(fill16(n * H * W).reshape(n, H, W, 1).copy()).to(ctx.device)
    before = dst.clone()
    out = torch.full((n, lib.dwtx_encode_bound16(W, H, 1)), FILL, dtype=torch.uint8, device=ctx.device)
    info = torch.full((n, C.sizeof(dwt_amd.StreamInfo)), FILL, dtype=torch.uint8, device=ctx.device)
    fsrc = src.float()
    fmt = dwt_amd.float_format(torch.float32)

    def refused(rc, word):
        text = lib.dwtx_last_error().decode()
        assert rc == ERR_ARG and word in text, (rc, word, text)   # (a text of this refusal's own, not an earlier one's)
        ctx.sync()
        assert (dst == before).all() and (out == FILL).all() and (info == FILL).all()

    def dec(view, minval, flip=0, step=0, order=0, f=None, cw=W, ch=H):
        infos = (dwt_amd.DecodeInfo * n)()
        return lib.dwtx_decode_view_signed(ctx.h, streams.data_ptr(), streams.shape[1], lens.data_ptr(), W, H, n, -1, C.byref(view), step, order, f,
                                           cw, ch, None, None, flip, None, minval, C.cast(infos, C.c_void_p))

    def enc(view, minval, flip=0, step=0, order=0, f=None):
        return lib.dwtx_encode_view_signed(ctx.h, C.byref(view), step, order, f, None, flip, None, minval, W, H, n, 0, out.data_ptr(), out.shape[1],
                                           info.data_ptr())

    def view(t, maxval=32767, **kw):
        v = dwt_amd.View(t.data_ptr(), t.element_size(), 1, maxval, 0, W, W * H, 0, 0)
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    # a range outside the rule
    for lo, hi in ((5, 5), (6, 5), (-32769, 100), (-5, 32768), (0, 40000)):
        refused(dec(view(dst, hi), lo), "range")
    for lo, hi in ((-32769, 100), (-5, 32768), (7, 7)):
        refused(enc(view(fsrc, hi), lo, f=C.byref(fmt)), "range")
        refused(dec(view(fsrc, hi), lo, f=C.byref(fmt)), "range")
    # one-byte samples without a float format
    refused(dec(view(dst, 255, sample_bytes=1), 0), "int16_t")
    refused(enc(view(src, 255, sample_bytes=1), 0), "int16_t")
    # what the flip calls refuse
    refused(dec(view(dst), -1024, flip=4), "flip")
    refused(enc(view(src), 0, flip=4), "flip")
    refused(dec(view(dst), -1024, order=7), "order")
    refused(enc(view(src), 0, order=2), "order")
    refused(dec(view(dst, row_pitch=W - 1), -1024), "row_pitch")
    refused(enc(view(src, row_pitch=W - 1), 0), "row_pitch")
    refused(dec(view(dst, image_stride=W * H - 1), -1024), "overlap")          # overlapping windows
    refused(dec(view(dst), -1024, cw=W + 1), "crop")                         # a crop that is no window of the picture
    refused(dec(view(dst, channels=2), -1024), "channels")
    refused(dec(view(dst), -1024, f=C.byref(fmt)), "float type")                   # sample_bytes does not match the float type
    # the keywords, before any device call
    with pytest.raises(ValueError):
        ctx.encode_view(src.view(torch.uint16) if hasattr(torch, "uint16") else src.byte(), signed=True)
    with pytest.raises(ValueError):
        ctx.decode_view(streams, lens, fsrc, signed=True)
    with pytest.raises(ValueError):
        ctx.decode_view(streams, lens, dst, minval=-5)
    # and the same call is taken once its argument is mended
    assert dec(view(dst, 3071), -1024) == 0
    assert (dst.cpu().numpy()[..., 0] == np.stack(pics)[..., 0]).all()


# ---- the host pair -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_the_host_pair(ctx, opts, wh, Cn):
    """dwtx_encode_images_s16 / dwtx_decode_images_s16, in parts of two, with CAPACITY and PIXELS."""
    W, H = wh
    lo, hi = -2048, 2047
    opts.set("part_images", 2)
    pics = pictures(W, H, Cn, lo, hi, 5)
    for capacity in (0, 700):
        streams, stats = ctx.encode16s(np.stack(pics), capacity)
        for p, s, st in zip(pics, streams, stats):
            want, ost = oracle_encode(p, capacity)
            assert s == want and (st.root_bits, st.total_bits, list(st.planes)[:Cn]) == (ost.root_bits, ost.total_bits, list(ost.planes)[:Cn])
    rows = decode_rows(W, H, Cn, lo, hi, 5)
    g = orc.geometry(W, H)
    for pixels_max in (-1, g.pixels[g.levels - 1], 0):
        got = ctx.decode16s(rows, lo, hi, pixels_max)
        for r, p in zip(rows, got):
            ref = signed.signed_decode(r, W, H, Cn, lo, hi, pixels_max)
            assert p.dtype == np.int16 and p.shape == ref.shape and (p == ref).all()
    single = ctx.decode16s(rows[0], lo, hi)
    assert (single == signed.signed_decode(rows[0], W, H, Cn, lo, hi)).all()
    with pytest.raises(Exception) as e:
        ctx.decode16s(rows, 5, 5)
    assert e.value.rc == ERR_ARG
    with pytest.raises(ValueError):
        ctx.encode16s(np.stack(pics).astype(np.uint16))


def test_the_host_pair_refuses_a_17_plane_picture(ctx):
    pics = np.stack([signed.noise(132, 72, 1, -32768, 32767, 4)])
    with pytest.raises(Exception) as e:
        ctx.encode16s(pics)
    assert e.value.rc == ERR_ARG and "16 bit planes" in str(e.value)


# ---- the sidecar index and the context's history -------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_the_encoders_index_of_a_signed_stream_is_taken_by_the_decode(ctx, opts, Cn):
    import torch

    import dwt_amd

    W, H, lo, hi = 132, 72, -1024, 3071
    pics = pictures(W, H, Cn, lo, hi, 3)
    t = torch.from_numpy(np.stack(pics)).to(ctx.device)
    dev_index = ctx.set_encode_index(3, device=True)
    try:
        out, info = ctx.encode_view(t, signed=True)
        enc = [dwt_amd.index_from_row(dev_index[i]) for i in range(3)]
    finally:
        ctx.set_encode_index()
    assert all(X.magic == dwt_amd.INDEX_MAGIC and X.nsegs > 0 and (X.W, X.H, X.C) == (W, H, Cn) for X in enc)
    lens = ctx.stream_lengths(info)
    into = torch.from_numpy(fill16(3 * H * W * Cn).reshape(3, H, W, Cn).copy()).to(ctx.device)
    opts.set("no_index_fallback", 1)   # (an index that is turned down is then an error)
    ctx.set_index((dwt_amd.Index * 3)(*enc), 0)
    try:
        infos = ctx.decode_view(out, lens, into, maxval=hi, minval=lo, signed=True)
    finally:
        ctx.set_index()
    assert [I.status for I in infos] == [0, 0, 0]
    assert (into.cpu().numpy() == np.stack(pics)).all()


def _unsigned_calls(ctx):
    """An unsigned deep encode and decode and a float decode on the shared context, each against the oracle."""
    import torch

    W, H, M = 132, 72, 4095
    pics = [deep.smooth_noise(W, H, 3, M, i + 1) for i in range(3)]
    t = V.to_device(ctx, np.stack(pics))
    out, info = ctx.encode_view(t)
    host = out.cpu().numpy()
    rows = []
    for i, I in enumerate(V.infos_of(info)):
        want = deep.deep_encode(pics[i])[0]
        assert host[i, :I.nbytes].tobytes() == want
        rows.append(want)
    rows[1] = rows[1][:len(rows[1]) // 2]
    streams, lens = to_streams(ctx, rows)
    into = torch.zeros((3, H, W, 3), dtype=torch.int16, device=ctx.device)
    ctx.decode_view(streams, lens, into, maxval=M)
    f = torch.zeros((3, 3, H, W), dtype=torch.float16, device=ctx.device)
    ctx.decode_view_float(streams, lens, f.permute(0, 2, 3, 1), maxval=M, scale=0.5, bias=1.0)
    for i, r in enumerate(rows):
        ref = deep.deep_decode(r, W, H, 3, M)
        assert (into[i].cpu().numpy().view(np.uint16) == ref).all()
        want = (torch.from_numpy(ref.astype(np.float32)) * 0.5 + 1.0).half()
        assert (f[i].permute(1, 2, 0).cpu() == want).all()


def _signed_calls(ctx):
    W, H = 132, 72
    for Cn in (1, 3):
        L = V.grid(W, H, Cn, "quad", rows=2, cols=2)
        check_encode(ctx, L, pictures(W, H, Cn, -2048, 2047, L.n), capacities=(0,))
        check_decode(ctx, L, W, H, Cn, decode_rows(W, H, Cn, -2048, 2047, L.n), -2048, 2047)


def test_results_do_not_depend_on_the_contexts_history(ctx):
    """A signed call after unsigned deep and float calls on one context, and the reverse (tests/history.py's concern: scratch
    slots, ring planes and tables that an earlier call of another kind left behind)."""
    _unsigned_calls(ctx)
    _signed_calls(ctx)
    _unsigned_calls(ctx)
    import dwt_amd

    fresh = dwt_amd.Context(0)
    try:
        _signed_calls(fresh)
        _unsigned_calls(fresh)
        _signed_calls(fresh)
    finally:
        fresh.close()
