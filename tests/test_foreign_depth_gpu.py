"""GPU: streams that no 8-bit picture makes through the 8-bit decoders — 15 and 16 bit planes, clamps at work.

bin/decode without DWTX_MAXVAL, dwtx_decode_images, dwtx_decode_device and the views decode any .dwt to bytes, "clamped at
255 as ever".  Fed by 8-bit pictures alone, three parts of that path never do anything visible: the clamps of the fused
inverse kernels (Y to [0,255], Co and Cg to [-255,255], then R, G, B to [0,255]), the `pmax <= 15` gate of unpack.hip's
scatter() that keeps a part of a batch off the 16-bit ring planes, and those planes beyond 11 bits.  The pictures here
(deep.impulses; tests/test_deep_cpu.py holds them to their plane counts, to coefficients of 32767 and to clamps that cut
about half of the samples) are encoded on the CPU by deep.deep_encode, so only the decoders are under test.

The yardstick is orc.decode, sample for sample, and the size it gives; for device buffers every sample of a prefilled
buffer, so that nothing outside the pictures, between the pixels of a stepped view or in a refused row's window changes."""
import numpy as np
import pytest

import deep
import orc
import test_deep_gpu as D
import test_planar_gpu as P
import test_step_gpu as S
import test_views_gpu as V

pytestmark = pytest.mark.gpu

GEOMETRIES = [(W, H, C) for W, H in deep.FOREIGN_WIDE + deep.FOREIGN_GENERAL for C in (1, 3)]
_refs = {}


def oracle(row):
    if row not in _refs:
        _refs[row] = orc.decode(row)
    return _refs[row]


def upload(ctx, rows):
    import torch

    stride = (max(len(r) for r in rows) + 64 + 7) // 8 * 8
    host = np.full((len(rows), stride), 0xA5, dtype=np.uint8)   # (live bytes past each stream's end)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return torch.from_numpy(host).to(ctx.device), torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)


def check_statuses(named, infos, W, H):
    g = orc.geometry(W, H)
    for (name, row), I in zip(named, infos):
        if name == deep.REFUSED:
            assert I.status == 2, name
            continue
        ref = oracle(row)
        assert I.status == 0 and (g.heights[I.level + 1], g.widths[I.level + 1]) == ref.shape[:2], name
        assert I.pmax == (int(name[:2]) if name[:2] in ("15", "16") else max(I.planes[:3])) and I.pmax <= 16, name


def check_device(ctx, named, W, H, Cn):
    """dwtx_decode_device into dense slots of a prefilled buffer: the oracle's picture at the start of each slot, at the
    oracle's size; the rest of the slot, a refused row's slot and the guard behind the last keep what was there."""
    import torch

    rows = [r for _, r in named]
    slot = W * H * Cn
    before = V.pattern(len(rows) * slot + D.GUARD, False)
    want = before.copy()
    for i, (name, row) in enumerate(named):
        if name != deep.REFUSED:
            ref = oracle(row)
            want[i * slot:i * slot + ref.size] = ref.reshape(-1)
    streams, lens = upload(ctx, rows)
    out = torch.from_numpy(before.copy()).to(ctx.device)
    _, infos = ctx.decode_device(streams, lens, W, H, Cn, out=out)
    check_statuses(named, infos, W, H)
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} samples differ, the first in row {bad[0] // slot} ({named[min(bad[0] // slot, len(named) - 1)][0]}) at {bad[0] % slot}"
    return got


def check_host(ctx, named):
    outs = ctx.decode([r for _, r in named])
    for (name, row), o in zip(named, outs):
        if name == deep.REFUSED:
            assert o is None, name
        else:
            ref = oracle(row)
            assert o is not None and o.shape == ref.shape and (o == ref).all(), name


def check_view(vctx, L, named, W, H):
    """decode_view into the windows of layout L (tests/test_views_gpu.py): the whole buffer afterwards."""
    assert L.n == len(named)
    buf = V.pattern(L.samples, False)
    want = buf.copy()
    for w, (name, row) in zip(L.np_windows(want), named):
        if name != deep.REFUSED:
            ref = oracle(row)
            w[:ref.shape[0], :ref.shape[1]] = ref
    streams, lens = upload(vctx, [r for _, r in named])
    tbuf = V.to_device(vctx, buf)
    infos = vctx.decode_view(streams, lens, L.t_view(tbuf))
    check_statuses(named, infos, W, H)
    bad = np.flatnonzero(tbuf.cpu().numpy() != want)
    assert bad.size == 0, f"{bad.size} samples differ, first at {bad[:5]} of {L.samples} (view offset {L.off}, strides {L.strides})"


# ---- every entry point ---------------------------------------------------------------------------------------------

BATCHES = {"clean": deep.foreign_clean_rows, "mixed": deep.foreign_rows}
ENTRIES = {1: ["host", "device", "window", "quad_window", "step2"], 3: ["host", "device", "window", "quad_window", "planar", "rgbx8"]}
CASES = [pytest.param(W, H, C, batch, entry, id="%dx%dx%d-%s-%s" % (W, H, C, batch, entry))
         for W, H, C in GEOMETRIES for batch in BATCHES for entry in ENTRIES[C]]


def on_the_quad_grid(L):
    """origin, pitch and every stride of the windows multiples of 4 samples: what the fused kernels ask of a view"""
    return L.off % 4 == 0 and all(s % 4 == 0 for s in L.strides[:-2])


@pytest.mark.parametrize("W,H,Cn,batch,entry", CASES)
def test_every_8_bit_decoder_on_deep_streams(ctx, W, H, Cn, batch, entry):
    """Two batches through each 8-bit entry point.  "clean" (deep.foreign_clean_rows): the 15-plane stream whose
    coefficients reach 32767, its 3/4 and 1/2 cuts (which reach the finest level: the dequantisation bias on large
    coefficients), an 8-bit picture's stream and two more 15-plane pictures — both decoder parts are whole and within 15
    planes, so at the wide shapes everything goes through the 16-bit ring planes, five levels of them at 1088x320, and
    the fused inverse kernels of the entry point read them.  "mixed" (deep.foreign_rows): 16-plane streams and their
    cuts, a cut that stops a level early and a stream that claims 17 planes beside them — no part takes the 16-bit planes,
    the fused kernels read int32 rings.  (tests/test_deep_cpu.py asserts both statements about the parts.)
    Entry points: dwtx_decode_images, dwtx_decode_device, dwtx_decode_view into interleaved windows with a pitch — off the
    quad grid (the general path) and on it (the fused kernels, at the wide shapes) —, planar windows and an RGBX8 surface
    (RGB), a plane with pixel step 2 (gray)."""
    named = BATCHES[batch](W, H, Cn)
    n = len(named)
    wide = (W, H) in deep.FOREIGN_WIDE
    if entry == "host":
        check_host(ctx, named)
    elif entry == "device":
        check_device(ctx, named, W, H, Cn)
    elif entry == "window":
        L = V.stack(W, H, Cn, n=n)
        assert not on_the_quad_grid(L)
        check_view(ctx, L, named, W, H)
    elif entry == "quad_window":
        L = V.grid(W, H, Cn, "quad", rows=n // 3, cols=3)
        assert on_the_quad_grid(L) or not wide
        check_view(ctx, L, named, W, H)
    elif entry == "planar":
        L = P.nchw(W, H, n=n)
        assert (L.off % 4 == 0 and all(s % 4 == 0 for s in (L.strides[0], L.strides[1], L.strides[3]))) or not wide
        check_view(ctx, L, named, W, H)
    elif entry == "rgbx8":
        L = S.sstack(W, H, 3, 4, n=n)
        assert L.off % 4 == 0 and all(s % 4 == 0 for s in L.strides[:-1])   # (what the 4-byte-pixel kernels ask)
        check_view(S.Stepped(ctx), L, named, W, H)
    else:
        check_view(S.Stepped(ctx), S.sstack(W, H, 1, 2, n=n), named, W, H)


@pytest.mark.parametrize("wh", deep.FOREIGN_WIDE, ids=lambda v: "%dx%d" % v)
def test_the_16_bit_ring_levels_are_the_ones_the_cpu_tests_assume(ctx, wh):
    """deep.levels16, on which tests/test_deep_cpu.py bases what it says about the 16-bit planes, is the mask the library
    reports; 1088x320 has five such levels and a sixth, the coarsest, in int32: the boundary lies inside the picture."""
    import torch

    W, H = wh
    for Cn in (1, 3):
        mask = ctx.transformation_fwd_pixels(torch.zeros((1, H, W, Cn), dtype=torch.uint8, device=ctx.device))[2]
        assert mask == deep.levels16(W, H) and mask != 0
    if wh == deep.FOREIGN_WIDE[-1]:
        assert bin(mask).count("1") == 5 and orc.geometry(W, H).levels == 6 and not mask & 1


# ---- batch composition: the gate is per part -----------------------------------------------------------------------

RUNS = [("decode_parts", 0), ("decode_parts", 2), ("decode_parts", 3), ("decode_parts", 4), ("one_stream", 1), ("no_fine16", 1),
        ("no_square_tiles", 1), ("lift_rows", 16), ("lift_rows", 64)]


@pytest.mark.parametrize("whc", deep.FOREIGN_BATCH_SHAPES, ids=lambda v: "%dx%dx%d" % v)
def test_a_16_plane_stream_among_others_however_the_batch_is_cut(ctx, opts, whc):
    """Twelve streams (deep.foreign_batch): cut into 2, 3 and 4 parts and run as one (`one_stream`), the 16-plane stream
    keeps different neighbours off the 16-bit ring planes while, from two parts on, another part takes them for the 32767
    stream (tests/test_deep_cpu.py) — every run gives the oracle's pixels, so all runs give identical ones; so do the runs
    without the 16-bit planes, without the tiles in the pyramid and with forced rows per wave.  (`decode_parts` 0, the
    automatic setting, is two parts for twelve rows: the same cut as 2, listed because it is what callers get.)  The
    refused row leaves its slot as it was."""
    W, H, Cn = whc
    named = deep.foreign_batch(W, H, Cn)
    first = None
    for name, value in RUNS:
        opts.set(name, value)
        got = check_device(ctx, named, W, H, Cn)
        first = got if first is None else first
        assert (got == first).all(), (name, value)
        opts.set(name, 0)


@pytest.mark.parametrize("planes", [15, 16])
@pytest.mark.parametrize("whc", deep.FOREIGN_BATCH_SHAPES, ids=lambda v: "%dx%dx%d" % v)
def test_uniform_batches_of_15_and_of_16_plane_streams(ctx, opts, whc, planes):
    """Six whole streams of one plane count, as two parts and as three: with 15 every part takes the 16-bit planes —
    coefficients up to 32767 in magnitude go through them, on five ring levels at 1088x320 —, with 16 none does."""
    W, H, Cn = whc
    named = deep.foreign_uniform(W, H, Cn, planes)
    for parts in (0, 3):
        opts.set("decode_parts", parts)
        check_device(ctx, named, W, H, Cn)
    check_host(ctx, named)


# ---- the same clamps in the deep outputs -----------------------------------------------------------------------------

@pytest.mark.parametrize("whc", [(256, 200, 3), (132, 72, 1), (131, 77, 3)], ids=lambda v: "%dx%dx%d" % v)
def test_decode16_with_a_maxval_below_the_datas(ctx, whc):
    """A maxval-4095 stream decoded with maxval 1023: the clamps of the deep outputs on whole streams, against
    deep.deep_decode(..., 1023); more than half of the samples are cut."""
    W, H, Cn = whc
    pic = deep.noise(W, H, Cn, 4095, 9)
    data = deep.deep_encode(pic)[0]
    assert (pic > 1023).mean() > 0.5
    refs = D._check_decodes(ctx, [data, data[:len(data) * 3 // 4], data[:len(data) // 2]], W, H, Cn, 1023)
    if Cn == 1:   # (the clamp is all that happens to a whole gray stream)
        assert (refs[0] == np.minimum(pic, 1023)).all()
