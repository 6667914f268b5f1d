"""GPU: delta views — dwtx_encode_view_delta / dwtx_decode_view_delta (include/dwtx.h): a picture coded as its difference
from a base view, both views where they lie.

The yardstick is the oracle on the CPU (tests/delta.py over tests/deep.py): deep_encode's bytes and counters of the integer
residual for every encode, delta_decode's samples for every decode.  Every comparison is exact and covers the WHOLE buffer: a
stream buffer is prefilled and must hold the oracle's bytes, the zero padding the contract names and the fill behind it; a
destination holds the oracle's picture in each written window and its fill pattern in every other sample; the base's buffer
is what it was.  Layouts are flat buffers of samples plus an offset, a shape and strides, as in tests/test_views_gpu.py; the
view and its base have a layout each.  n is 3 to 5."""
import numpy as np
import pytest

import deep
import delta
import levels
import orc
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
# 132x72 and 520x264: W % 4 == 0 and more than 64 on a side (one and two wide levels of the transform); 263x135: W % 4 != 0
SHAPES = delta.SHAPES
FILL = 0xA5
# kind -> (minval, maxval, numpy dtype, signed=)
KINDS = {"u8": (0, 255, np.uint8, False), "u16": (0, 4095, np.uint16, False), "s16": (-1024, 3071, np.int16, True)}
KIND_NAMES = list(KINDS)


# ---- layouts: (view's Layout, base's Layout, stepped) by name; all strides in samples -------------------------------------------

def dense(W, H, Cn, n=3):
    return V.Layout(n * H * W * Cn, 0, (n, H, W, Cn), (H * W * Cn, W * Cn, Cn, 1))


def nchw(W, H, n=3, off=8):
    img = 3 * H * W + 12
    return V.Layout(off + n * img + 5, off, (n, H, W, 3), (img, W, 1, H * W + 4))


def stepped(W, H, Cn, step, n=3):
    pitch = W * step + 4
    return V.Layout(4 + n * H * pitch, 4, (n, H, W, Cn), (H * pitch, pitch, step, 1))


LAYOUTS = {
    "dense-dense": lambda W, H, Cn: (dense(W, H, Cn), dense(W, H, Cn), False),
    "pitched-dense": lambda W, H, Cn: (V.grid(W, H, Cn, "quad", rows=2, cols=2), dense(W, H, Cn, 4), False),      # windows on the quad
    "off1-dense": lambda W, H, Cn: (V.grid(W, H, Cn, "off1", rows=2, cols=2), dense(W, H, Cn, 4), False),         # one column off it
    "dense-stack": lambda W, H, Cn: (dense(W, H, Cn), V.stack(W, H, Cn), False),                                  # a pitched base
    "tiles-tiles": lambda W, H, Cn: (V.grid(W, H, Cn, "quad", rows=2, cols=2), V.grid(W, H, Cn, "pitch", rows=2, cols=2), False),
    "planar-dense": lambda W, H, Cn: (nchw(W, H), dense(W, H, 3), False),                                         # (RGB only: LAYOUT_CASES)
    "dense-planar": lambda W, H, Cn: (dense(W, H, 3), nchw(W, H), False),
    "planar-planar": lambda W, H, Cn: (nchw(W, H), nchw(W, H, off=4), False),
    "step-dense": lambda W, H, Cn: (stepped(W, H, Cn, 4 if Cn == 3 else 2), dense(W, H, Cn), True),               # RGBX-style step 4, gray step 2
    "dense-step": lambda W, H, Cn: (dense(W, H, Cn), stepped(W, H, Cn, 4 if Cn == 3 else 2), True),
}

LAYOUT_CASES = [(wh, Cn, layout) for wh in SHAPES for Cn in (1, 3) for layout in LAYOUTS if Cn == 3 or "planar" not in layout]
_case_id = lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], "gray" if c[1] == 1 else "rgb", c[2])   # noqa: E731


def kind_of(case):
    """Every (channels, layout) meets the three sample types over the three shapes."""
    (W, H), Cn, layout = case
    return KIND_NAMES[(SHAPES.index((W, H)) + list(LAYOUTS).index(layout) + Cn) % 3]


def fill(samples, dt, salt=0):
    """A buffer's fill: values all over the sample type."""
    i = np.arange(samples, dtype=np.int64) + salt * 1001
    v = i * 7919 + (i >> 7) * 13
    return (v % 251).astype(np.uint8) if dt == np.uint8 else (v % 65521).astype(np.uint16).view(dt)


def in_memory(pic, order):
    return pic[..., ::-1] if order == "bgr" else pic


def pairs(W, H, Cn, kind, n):
    """n pairs (S, B): successor frames, one pair of block pictures (residuals of -R, 0 and R) among them."""
    lo, hi = KINDS[kind][:2]
    out = [delta.successor(W, H, Cn, lo, hi, i + 1) for i in range(n)]
    out[1] = delta.clamp_pair(W, H, Cn, lo, hi)
    return out


# ---- encode ------------------------------------------------------------------------------------------------------------------------

def check_streams(out, info, prs, capacity=0, refused=(), prefilled=True):
    """The whole stream buffer (prefilled with FILL) and the records against the oracle on the residuals."""
    host = out.cpu().numpy()
    infos = V.infos_of(info)
    stride = host.shape[1]
    for i, (S, B) in enumerate(prs):
        I = infos[i]
        if i in refused:
            assert I.error == 1, i
            continue
        want, st = delta.stream(S, B, capacity)
        Cn = S.shape[2]
        assert I.error == 0 and I.nbytes == len(want), (i, I.error, I.nbytes, len(want))
        assert host[i, :I.nbytes].tobytes() == want, i
        assert list(I.planes)[:Cn] == list(st.planes)[:Cn] and (I.root_bits, I.total_bits) == (st.root_bits, st.total_bits), i
        if capacity <= 0:   # (the zero padding after a stream that CAPACITY does not cut, and the slot's bytes beyond left as they were)
            pad = min(stride, (I.nbytes + 3) // 4 * 4 + 16)
            assert not host[i, I.nbytes:pad].any(), i
            assert not prefilled or (host[i, pad:] == FILL).all(), i


def load(ctx, L, pics, dt, order="rgb", salt=0):
    """-> (the host buffer with pics in L's windows, its device copy)."""
    buf = fill(L.samples, dt, salt)
    for w, p in zip(L.np_windows(buf), pics):
        w[...] = in_memory(p, order)
    return buf, V.to_device(ctx, buf)


def check_encode(ctx, kind, Ls, Lb, prs, stepped=False, order="rgb", capacities=(0, 500), refused=()):
    import torch

    lo, hi, dt, sgn = KINDS[kind] if isinstance(kind, str) else kind
    H, W, Cn = prs[0][0].shape
    bufS, tS = load(ctx, Ls, [p[0] for p in prs], dt, order)
    bufB, tB = load(ctx, Lb, [p[1] for p in prs], dt, order, salt=1)
    stride = ctx.lib.dwtx_encode_bound16(W, H, Cn)
    for capacity in capacities:
        out = torch.full((Ls.n, stride if capacity <= 0 else (capacity + 15) // 8 * 8), FILL, dtype=torch.uint8, device=ctx.device)
        out, info = ctx.encode_view(Ls.t_view(tS), capacity, out=out, stepped=stepped, order=order, signed=sgn, base=Lb.t_view(tB))
        check_streams(out, info, prs, capacity, refused)
    assert (V.to_host(tS, dt == np.uint16) == bufS).all() and (V.to_host(tB, dt == np.uint16) == bufB).all(), "a source was written to"
    return out, info


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_case_id)
def test_delta_encode_equals_the_oracle(ctx, opts, case):
    """Every pair of layouts, with and without NO_PIXELS16."""
    (W, H), Cn, layout = case
    Ls, Lb, stp = LAYOUTS[layout](W, H, Cn)
    kind = kind_of(case)
    check_encode(ctx, kind, Ls, Lb, pairs(W, H, Cn, kind, Ls.n), stepped=stp)
    opts.set("no_pixels16", 1)
    check_encode(ctx, kind, Ls, Lb, pairs(W, H, Cn, kind, Ls.n), stepped=stp, capacities=(0,))


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_delta_encode_of_every_sample_type_dense(ctx, kind, Cn):
    W, H = 132, 72
    check_encode(ctx, kind, dense(W, H, Cn, 4), dense(W, H, Cn, 4), pairs(W, H, Cn, kind, 4), capacities=(0,))


@pytest.mark.parametrize("layout", ["dense-dense", "planar-dense", "planar-planar", "step-dense"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_delta_encode_of_bgr_pixels(ctx, wh, layout):
    W, H = wh
    Ls, Lb, stp = LAYOUTS[layout](W, H, 3)
    kind = KIND_NAMES[(SHAPES.index(wh) + len(layout)) % 3]
    check_encode(ctx, kind, Ls, Lb, pairs(W, H, 3, kind, Ls.n), stepped=stp, order="bgr", capacities=(0,))


def chain(W, H, Cn, kind, n):
    """n + 1 frames, each the successor of the one before."""
    lo, hi = KINDS[kind][:2]
    rng = np.random.default_rng(77)
    frames = [delta.successor(W, H, Cn, lo, hi, 2)[1]]
    for i in range(n):
        f = frames[-1].astype(np.int64)
        g = f + rng.integers(-2, 3, f.shape)
        g[20 + i:52 + i, 30 + 2 * i:70 + 2 * i] = f[18:50, 27:67]
        frames.append(np.clip(g, lo, hi).astype(frames[0].dtype))
    return frames


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_delta_encode_of_a_stack_against_itself(ctx, wh, Cn, kind):
    """`t[1:]` against `t[:-1]`: the two views overlap in all frames but two; both are only read."""
    import torch

    W, H = wh
    n = 4
    lo, hi, dt, sgn = KINDS[kind]
    frames = chain(W, H, Cn, kind, n)
    t = V.to_device(ctx, np.stack(frames))
    out = torch.full((n, ctx.lib.dwtx_encode_bound16(W, H, Cn)), FILL, dtype=torch.uint8, device=ctx.device)
    out, info = ctx.encode_view(t[1:], out=out, signed=sgn, base=t[:-1])
    check_streams(out, info, [(frames[i + 1], frames[i]) for i in range(n)])
    assert (V.to_host(t, dt == np.uint16) == np.stack(frames)).all()


@pytest.mark.parametrize("option", ["no_square_tiles", "exact_orders", "one_stream"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_delta_encode_under_the_switches(ctx, opts, wh, option):
    W, H = wh
    opts.set(option, 1)
    for Cn, kind in ((1, "u8"), (3, "s16"), (3, "u8")):
        Ls, Lb, _ = LAYOUTS["pitched-dense"](W, H, Cn)
        check_encode(ctx, kind, Ls, Lb, pairs(W, H, Cn, kind, Ls.n), capacities=(0, 700))


@pytest.mark.parametrize("rows_per_wave", [4, 16, 64])
def test_delta_at_the_strip_edges(ctx, opts, rows_per_wave):
    """260x131 under every strip height — a width one lane into a second strip, a last row pair without its odd row —, encode and
    decode, gray, interleaved and planar, with and without NO_PIXELS16."""
    W, H = 260, 131
    opts.set("lift_rows", rows_per_wave)
    for no16 in (0, 1):
        opts.set("no_pixels16", no16)
        for Cn, kind, Ls, Lb, order in ((1, "u8", V.grid(W, H, 1, "quad", rows=2, cols=2), dense(W, H, 1, 4), "rgb"),
                                        (1, "s16", dense(W, H, 1, 4), dense(W, H, 1, 4), "rgb"),
                                        (3, "u8", dense(W, H, 3, 4), dense(W, H, 3, 4), "bgr"), (3, "u16", nchw(W, H, 4), nchw(W, H, 4, off=4), "rgb")):
            prs = pairs(W, H, Cn, kind, 4)
            check_encode(ctx, kind, Ls, Lb, prs, order=order, capacities=(0,))
            check_decode(ctx, kind, Ls, Lb, decode_rows(W, H, Cn, kind, 4), order=order)


def test_a_zero_base_gives_the_plain_calls_bytes_and_samples(ctx):
    import torch

    W, H = 132, 72
    for kind, Cn in (("u8", 3), ("u16", 1), ("s16", 3)):
        lo, hi, dt, sgn = KINDS[kind]
        pics = [delta.successor(W, H, Cn, lo, hi, i)[0] for i in range(3)]
        t = V.to_device(ctx, np.stack(pics))
        zero = torch.zeros_like(t)
        plain, pinfo = ctx.encode_view(t, signed=sgn)
        out, info = ctx.encode_view(t, signed=sgn, base=zero)
        lens = ctx.stream_lengths(info)
        assert (lens == ctx.stream_lengths(pinfo)).all()
        for i in range(3):
            k = int(lens[i])
            assert (out[i, :k] == plain[i, :k]).all()
        a, b = torch.zeros_like(t), torch.zeros_like(t)
        ia = ctx.decode_view(plain, lens, a, maxval=hi, signed=sgn, minval=lo if sgn else None)
        ib = ctx.decode_view(out, lens, b, maxval=hi, signed=sgn, minval=lo if sgn else None, base=zero)
        assert [I.status for I in ia] == [I.status for I in ib] == [0, 0, 0]
        assert (a == b).all() and (V.to_host(b, dt == np.uint16) == np.stack(pics)).all()


@pytest.mark.parametrize("sgn", [0, 1], ids=["uint16", "int16"])
def test_full_range_pictures(ctx, sgn):
    """Full-range pictures whose residuals leave int16 are coded and come back exactly; the residual of two noise pictures
    (18 planes) is refused alone in its batch."""
    import torch

    W, H = 132, 72
    kind = (-32768, 32767, np.int16, True) if sgn else (0, 65535, np.uint16, False)
    prs = [delta.full_range_pair(W, H, sgn, 0), delta.noise_pair(W, H, sgn), delta.full_range_pair(W, H, sgn, 1)]
    assert delta.stream(*prs[1])[1].planes[0] > 16
    L = dense(W, H, 1)
    out, info = check_encode(ctx, kind, L, L, prs, capacities=(0,), refused={1})
    lens = ctx.stream_lengths(info)
    keep = [0, 2]
    streams, lens = out[keep].contiguous(), lens[keep].contiguous()
    tB = V.to_device(ctx, np.stack([prs[i][1] for i in keep]))
    into = torch.zeros_like(tB)
    infos = ctx.decode_view(streams, lens, into, maxval=kind[1], signed=bool(sgn), minval=kind[0] if sgn else None, base=tB)
    assert [I.status for I in infos] == [0, 0]
    assert (V.to_host(into, not sgn) == np.stack([prs[i][0] for i in keep])).all()


# ---- decode ------------------------------------------------------------------------------------------------------------------------

def to_streams(ctx, rows):
    import torch

    stride = (max(len(r) for r in rows) + 64 + 7) // 8 * 8
    host = np.full((len(rows), stride), FILL, dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return torch.from_numpy(host).to(ctx.device), torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)


def decode_rows(W, H, Cn, kind, n):
    """n rows (stream, base): a whole successor stream, the two cut clamp fixtures, whole streams."""
    lo, hi = KINDS[kind][:2]
    rows = []
    for i in range(n):
        if i in (1, 2):
            rows.append(delta.cut_fixture(W, H, Cn, lo, hi, delta.CUTS[i - 1]))
        else:
            S, B = delta.successor(W, H, Cn, lo, hi, i + 1)
            rows.append((delta.stream(S, B)[0], B))
    return rows


_decoded = {}


def oracle_decode(data, B, W, H, Cn, lo, hi):
    key = (data, B.tobytes(), W, H, Cn, lo, hi)
    if key not in _decoded:
        _decoded[key] = delta.delta_decode(data, B, W, H, Cn, lo, hi)
    return _decoded[key]


def check_decode(ctx, kind, Ld, Lb, rows, stepped=False, order="rgb", in_place=False):
    """rows: (stream, base picture) per window.  The whole destination buffer and the whole base buffer afterwards.  in_place:
    the bases lie in the destination's windows and base= is the destination."""
    lo, hi, dt, sgn = KINDS[kind] if isinstance(kind, str) else kind
    H, W, Cn = rows[0][1].shape
    refs = [oracle_decode(r, B, W, H, Cn, lo, hi) for r, B in rows]
    if in_place:
        buf, tbuf = load(ctx, Ld, [B for _, B in rows], dt, order)
        tbase = tbuf
    else:
        buf = fill(Ld.samples, dt)
        tbuf = V.to_device(ctx, buf)
        bufB, tbase = load(ctx, Lb, [B for _, B in rows], dt, order, salt=1)
    want = buf.copy()
    for w, ref in zip(Ld.np_windows(want), refs):
        if ref is not None and ref is not delta.UNTOUCHED:
            w[...] = in_memory(ref, order)
    streams, lens = to_streams(ctx, [r for r, _ in rows])
    tv = Ld.t_view(tbuf)
    infos = ctx.decode_view(streams, lens, tv, maxval=hi, stepped=stepped, order=order, signed=sgn, minval=lo if sgn else None,
                            base=tv if in_place else Lb.t_view(tbase))
    T = orc.geometry(W, H).levels
    for (r, _), ref, I in zip(rows, refs, infos):
        if ref is None:
            assert I.status != 0
        else:
            assert I.status == 0 and (I.level == T - 1) == (ref is not delta.UNTOUCHED), (I.status, I.level)
    got = V.to_host(tbuf, dt == np.uint16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
    if not in_place:
        assert (V.to_host(tbase, dt == np.uint16) == bufB).all(), "the base was written to"
    return infos


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_case_id)
def test_delta_decode_equals_the_oracle(ctx, opts, case):
    """Whole streams back to S and the cut fixtures against delta_decode, into every sink, with and without NO_PIXELS16."""
    (W, H), Cn, layout = case
    Ld, Lb, stp = LAYOUTS[layout](W, H, Cn)
    kind = kind_of(case)
    check_decode(ctx, kind, Ld, Lb, decode_rows(W, H, Cn, kind, Ld.n), stepped=stp)
    opts.set("no_pixels16", 1)
    check_decode(ctx, kind, Ld, Lb, decode_rows(W, H, Cn, kind, Ld.n), stepped=stp)


@pytest.mark.parametrize("layout", ["dense-dense", "planar-dense", "step-dense"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_delta_decode_of_bgr_pixels(ctx, wh, layout):
    W, H = wh
    Ld, Lb, stp = LAYOUTS[layout](W, H, 3)
    kind = KIND_NAMES[(SHAPES.index(wh) + len(layout)) % 3]
    check_decode(ctx, kind, Ld, Lb, decode_rows(W, H, 3, kind, Ld.n), stepped=stp, order="bgr")


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_delta_decode_in_place(ctx, wh, Cn, kind):
    W, H = wh
    for L, stp in ((dense(W, H, Cn, 4), False), (V.grid(W, H, Cn, "off1", rows=2, cols=2), False)) + (((nchw(W, H, 4), False),) if Cn == 3 else ()):
        check_decode(ctx, kind, L, L, decode_rows(W, H, Cn, kind, 4), stepped=stp, in_place=True)


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_unreadable_and_reduced_streams_leave_their_windows(ctx, wh, Cn):
    """One stream that nothing reads and one cut just below its finest level: both windows untouched, the neighbours written."""
    W, H = wh
    kind = KIND_NAMES[(SHAPES.index(wh) + Cn) % 3]
    lo, hi = KINDS[kind][:2]
    rows = decode_rows(W, H, Cn, kind, 5)
    T = orc.geometry(W, H).levels
    S, B = delta.clamp_pair(W, H, Cn, lo, hi)
    rows[1] = (delta.stream(S, B)[0][:5], B)
    rows[3] = (levels.late_prefix(delta.stream(S, B)[0], W, H, Cn, T - 2), B)
    assert oracle_decode(rows[1][0], B, W, H, Cn, lo, hi) is None and oracle_decode(rows[3][0], B, W, H, Cn, lo, hi) is delta.UNTOUCHED
    infos = check_decode(ctx, kind, V.stack(W, H, Cn, 5), dense(W, H, Cn, 5), rows)
    assert infos[1].status != 0 and infos[3].status == 0 and infos[3].level == T - 2
    check_decode(ctx, kind, dense(W, H, Cn, 5), None, rows, in_place=True)


@pytest.mark.parametrize("option,value", [("decode_parts", 2), ("decode_parts", 4), ("one_stream", 1)])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_delta_decode_in_parts(ctx, opts, wh, option, value):
    W, H = wh
    opts.set(option, value)
    for Cn, kind in ((1, "u16"), (3, "u8")):
        rows = decode_rows(W, H, Cn, kind, 5)
        lo, hi = KINDS[kind][:2]
        S, B = delta.clamp_pair(W, H, Cn, lo, hi)
        rows[3] = (levels.late_prefix(delta.stream(S, B)[0], W, H, Cn, orc.geometry(W, H).levels - 2), B)
        check_decode(ctx, kind, V.stack(W, H, Cn, 5), V.stack(W, H, Cn, 5), rows)


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_the_encoders_index_of_a_delta_stream_is_taken_by_the_decode(ctx, opts, Cn):
    import torch

    import dwt_amd

    W, H, kind = 132, 72, "u8"
    lo, hi, dt, sgn = KINDS[kind]
    prs = pairs(W, H, Cn, kind, 3)
    tS, tB = (V.to_device(ctx, np.stack([p[k] for p in prs])) for k in (0, 1))
    dev_index = ctx.set_encode_index(3, device=True)
    try:
        out, info = ctx.encode_view(tS, base=tB)
        enc = [dwt_amd.index_from_row(dev_index[i]) for i in range(3)]
    finally:
        ctx.set_encode_index()
    assert all(X.magic == dwt_amd.INDEX_MAGIC and X.nsegs > 0 and (X.W, X.H, X.C) == (W, H, Cn) for X in enc)
    check_streams(out, info, prs, prefilled=False)
    lens = ctx.stream_lengths(info)
    into = torch.zeros_like(tS)
    opts.set("no_index_fallback", 1)   # (an index that is turned down is then an error)
    ctx.set_index((dwt_amd.Index * 3)(*enc), 0)
    try:
        infos = ctx.decode_view(out, lens, into, base=tB)
    finally:
        ctx.set_index()
    assert [I.status for I in infos] == [0, 0, 0]
    assert (into == tS).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_with_their_texts_and_nothing_written(ctx):
    import torch

    import dwt_amd

    W, H, n = 132, 72, 3
    t = torch.full((n + 1, H, W, 1), 7, dtype=torch.uint8, device=ctx.device)
    other = torch.full((n, H, W, 1), 9, dtype=torch.uint8, device=ctx.device)
    streams = torch.zeros((n, 4096), dtype=torch.uint8, device=ctx.device)
    lens = torch.full((n,), 100, dtype=torch.int64, device=ctx.device)

    def refused(text, fn):
        with pytest.raises(dwt_amd.DwtxError) as e:
            fn()
        assert e.value.rc == ERR_ARG and text in str(e.value), str(e.value)

    # a chain is no decode; one row down neither
    refused("meets window", lambda: ctx.decode_view(streams, lens, t[1:], base=t[:-1]))
    flat = t.reshape(-1)
    shifted = flat.as_strided((n, H, W, 1), (H * W, W, 1, 1), W)
    refused("meets window", lambda: ctx.decode_view(streams, lens, t[:-1], base=shifted))
    # 8-bit samples have one maxval; a signed range must be one
    refused("maxval 100", lambda: ctx.decode_view(streams, lens, other, maxval=100, base=t[:-1]))
    s16 = torch.zeros((n, H, W, 1), dtype=torch.int16, device=ctx.device)
    refused("minval < maxval", lambda: ctx.decode_view(streams, lens, s16, signed=True, minval=50, maxval=10, base=torch.zeros_like(s16)))
    assert (t == 7).all() and (other == 9).all() and not s16.any()
    # before any device call
    for bad in (dict(base=other.to(torch.int16)), dict(base=other[:, :, :64]), dict(base=other.float()), dict(base=other, flip="y")):
        with pytest.raises(ValueError):
            ctx.encode_view(other, **bad)
        with pytest.raises(ValueError):
            ctx.decode_view(streams, lens, other, **bad)
    with pytest.raises(ValueError):
        ctx.decode_view(streams, lens, other, base=t[:-1], levels_max=2)
    with pytest.raises(ValueError):
        ctx.encode_view(other.float(), base=other.float())
    assert (other == 9).all()


# ---- the context's history and tiles -----------------------------------------------------------------------------------------------

def test_delta_calls_between_plain_calls_of_other_geometry(ctx):
    """A delta call right after plain calls of another geometry on the same context, and a plain call after it."""
    def plain(W, H, Cn):
        V.check_encode(ctx, dense(W, H, Cn), W, H, Cn, False, capacities=(0,))
        V.check_encode(ctx, V.grid(W, H, Cn, "quad", rows=2, cols=2), W, H, Cn, True, capacities=(0,))

    plain(256, 256, 3)
    W, H = 132, 72
    for Cn, kind in ((3, "u8"), (1, "s16")):
        Ls, Lb, _ = LAYOUTS["pitched-dense"](W, H, Cn)
        check_encode(ctx, kind, Ls, Lb, pairs(W, H, Cn, kind, Ls.n), capacities=(0,))
        check_decode(ctx, kind, Ls, Lb, decode_rows(W, H, Cn, kind, Ls.n))
        plain(72, 68, Cn)
        check_decode(ctx, kind, Ls, Lb, decode_rows(W, H, Cn, kind, Ls.n), in_place=True)
    plain(132, 100, 1)


@pytest.mark.parametrize("kind", ["u8", "s16"])
def test_tiles_round_trip_with_a_base(ctx, kind):
    import torch

    from dwt_amd import tiles

    W, H, Cn, tile = 300, 200, 3, 128
    lo, hi, dt, sgn = KINDS[kind]
    S, B = delta.successor(W, H, Cn, lo, hi, 3)
    tS, tB = V.to_device(ctx, S), V.to_device(ctx, B)
    if sgn:   # (tiles.py has no signed keyword: the frames travel through the view calls by hand)
        groups = []
        for g in dwt_amd_groups(W, H, tile):
            out, info = ctx.encode_view(tiles.group_view(tS, g), signed=True, base=tiles.group_view(tB, g))
            groups.append((g, out, ctx.stream_lengths(info), info))
        into = torch.zeros_like(tS)
        for g, out, lens, _ in groups:
            infos = ctx.decode_view(out, lens, tiles.group_view(into, g), maxval=hi, signed=True, minval=lo, base=tiles.group_view(tB, g))
            assert all(I.status == 0 for I in infos)
        assert (into == tS).all()
        return
    groups = tiles.encode_frame(ctx, tS, tile, base=tB)
    plain = tiles.encode_frame(ctx, tS, tile)
    assert sum(int(g[2].sum()) for g in groups) < sum(int(g[2].sum()) for g in plain)
    for g, out, lens, info in groups:
        view = tiles.group_view(tS, g).reshape(-1, g.H, g.W, Cn).cpu().numpy()
        bview = tiles.group_view(tB, g).reshape(-1, g.H, g.W, Cn).cpu().numpy()
        check_streams(out, info, list(zip(view, bview)), prefilled=False)
    into = torch.zeros_like(tS)
    for infos in tiles.decode_frame(ctx, groups, into, base=tB):
        assert all(I.status == 0 for I in infos)
    assert (into == tS).all()
    # in place: the base frame becomes the picture
    work = tB.clone()
    tiles.decode_frame(ctx, groups, work, base=work)
    assert (work == tS).all() and (tB.cpu().numpy() == B).all()
    with pytest.raises(ValueError):
        tiles.encode_frame(ctx, tS, tile, base=tB[:-1])


def dwt_amd_groups(W, H, tile):
    import dwt_amd

    return dwt_amd.tile_groups(W, H, tile)
