"""GPU: the decoder's ones count leaves out the (ring, plane) segments in which no one was set (unpack.hip: seg_ones,
k_rank, k_count).  DWTX_OPT_COUNT_EVERY_PLANE ("count_every_plane") counts every segment as before:
every case here decodes with the switch off and on, and both must give what the oracle decodes — coefficients or
pixels, the decode info and the status.  A flag that is missing where a one was set would lose that coefficient.
(Checked once with builds that leave one of the stores out: without the walker's, 13 of the 19 cases fail, without the one
of k_hopbits' per-thread rows 17; without the one of its workgroup window none does — a stitched stretch begins and ends
inside chunks whose pieces go through the per-thread rows and raise the same flag, so no stream shows that store alone.)"""
import ctypes
import functools

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("status", "level", "nsegs", "truncated", "pmax", "bits_used", "zeros_left")


def _decode(ctx, streams, W, H, Cn):
    lin, infos = ctx.decode_planes(streams, W, H, Cn)
    lin = lin.cpu().numpy().reshape(len(streams), Cn, W * H)
    for i, info in enumerate(infos):
        if info.status:
            lin[i] = 0   # nothing is written for an unreadable stream
    return lin, infos


@functools.lru_cache(maxsize=None)
def _oracle(data, W, H, Cn):
    return orc.decode_stage(data, W, H, Cn, -1)


def both_ways(ctx, opts, streams, W, H, Cn, whole=None):
    """Decodes `streams` with the switch off and on: the two agree, and both agree with the oracle's decode of every
    stream (tests/test_unpack_gpu.py check()).  whole: the planes the streams were made of, which must come back."""
    runs = []
    for every in (0, 1):
        opts.set("count_every_plane", every)
        runs.append(_decode(ctx, streams, W, H, Cn))
    opts.set("count_every_plane", 0)
    (skip, sinfos), (every, einfos) = runs
    for i, (a, b) in enumerate(zip(sinfos, einfos)):
        for f in INFO_FIELDS:
            assert getattr(a, f) == getattr(b, f), (i, f)
        assert list(a.planes) == list(b.planes) and list(a.missing) == list(b.missing), i
    assert (skip == every).all()
    for i, data in enumerate(streams):
        ref = _oracle(data, W, H, Cn)
        for lin, infos in runs:
            if ref is None:
                assert infos[i].status == 1, i
                continue
            rlin, level, missing, planes = ref
            if max(planes) > 16:   # the documented difference
                assert infos[i].status == 2, i
                continue
            assert infos[i].status == 0, i
            assert list(infos[i].planes)[:Cn] == planes, i
            assert infos[i].level == level, i
            assert list(infos[i].missing) == missing.tolist(), i
            assert (lin[i] == rlin).all(), i
            if whole is not None:
                assert not infos[i].truncated and (lin[i] == whole[i]).all(), i
    return runs[0]


# ---- pictures -----------------------------------------------------------------------------------------------

def _bright_pixel(W, H):
    pix = np.zeros((H, W, 1), dtype=np.uint8)
    pix[H // 3, W // 2, 0] = 255
    return pix


PICTURES = {
    "synth 128x128x1": lambda: orc.synth(128, 128, 1, 41, 0),
    "synth 256x192x1": lambda: orc.synth(256, 192, 1, 42, 0),
    "synth 96x64x3": lambda: orc.synth(96, 64, 3, 43, 0),
    "synth 260x516x1": lambda: orc.synth(260, 516, 1, 44, 0),   # tiles cut by ring edges
    "synth 512x512x1": lambda: orc.synth(512, 512, 1, 45, 0),
    "flat 256x192x1": lambda: np.full((192, 256, 1), 77, dtype=np.uint8),
    "flat 96x64x3": lambda: np.full((64, 96, 3), 200, dtype=np.uint8),
    "one bright pixel 256x192x1": lambda: _bright_pixel(256, 192),
    "one bright pixel 512x512x1": lambda: _bright_pixel(512, 512),
}


@pytest.mark.parametrize("name", list(PICTURES))
def test_pictures(ctx, opts, name):
    """Alone (one or two images take both path families) and three times in a batch (one family); coefficients against
    orc.decode_stage, pixels against orc.decode."""
    pix = PICTURES[name]()
    H, W, Cn = pix.shape
    data, _ = orc.encode(pix)
    both_ways(ctx, opts, [data], W, H, Cn)
    both_ways(ctx, opts, [data, data, data], W, H, Cn)
    want = orc.decode(data)   # (a flat picture comes back smaller: the reference's quirk, the decoder's too)
    for every in (0, 1):
        opts.set("count_every_plane", every)
        got = ctx.decode(data)
        assert got.shape == want.shape and (got == want).all()


# ---- crafted coefficient planes ------------------------------------------------------------------------------

W0 = H0 = 512


@functools.lru_cache(maxsize=None)
def _rings():
    g = orc.geometry(W0, H0)
    return g.levels, [g.pixels[l] for l in range(g.levels + 1)]


def _base(nplanes, seed, quiet_rings=1):
    """Coefficients of a picture with `nplanes` bit planes whose `quiet_rings` finest rings are all zero"""
    levels, px = _rings()
    rng = np.random.default_rng(seed)
    lin = np.zeros((1, W0 * H0), dtype=np.int32)
    n = px[levels - quiet_rings]
    lin[0, :n] = rng.laplace(0.0, 3.0, n).astype(np.int32).clip(-40, 40)
    lin[0, px[1]] = (1 << nplanes) - 1   # fixes the plane count
    return lin


@functools.lru_cache(maxsize=None)
def crafted(nplanes):
    """-> (names, planes [n, 1, W*H], streams): the finest ring (196 608 symbols, 192 tiles) holds nothing but one
    coefficient of magnitude 2^p — every segment of the ring but one holds no one at all — at the ring's first and
    last position, at a tile's last and the next tile's first, for p at the top plane, in the middle and at plane 0;
    then the special cases."""
    levels, px = _rings()
    r0, r1 = px[levels - 1], px[levels]
    names, planes = [], []
    top, mid = nplanes - 1, nplanes // 2
    spots = {"ring's first": 0, "ring's last": r1 - r0 - 1, "tile's last": 37 * 1024 + 1023, "next tile's first": 38 * 1024}
    for p in (top, mid, 0):
        for what, at in spots.items():
            lin = _base(nplanes, 100 + p)
            lin[0, r0 + at] = (1 << p) * (-1 if at & 1 else 1)
            names.append(f"{nplanes} planes, 2^{p} at the {what}")
            planes.append(lin)
    # A zero run longer than k_hopbits' window of 32768 symbols that starts inside the segment: the ring's first coefficient
    # is significant from the top plane on, so every later segment of the ring ends with a refinement block (runs do not
    # straddle it, rle.h:95-101) and begins with a fresh token, whose run reaches the one 150 000 symbols further on
    for p in (mid, 0):
        lin = _base(nplanes, 200 + p)
        lin[0, r0] = 1 << top
        lin[0, r0 + 150000] = -(1 << p)
        names.append(f"{nplanes} planes, 2^{p} behind a run of 150 000 zeros")
        planes.append(lin)
    # among dense neighbours: the ring is full of small coefficients (planes 0 and 1 dense: whole workgroups of
    # k_hopbits inside one stitched run), the planes above hold the one coefficient only
    for p in (top, mid):
        lin = _base(nplanes, 300 + p)
        rng = np.random.default_rng(300 + p)
        lin[0, r0:r1] = rng.integers(-3, 4, r1 - r0)
        lin[0, r0 + 77777] = 1 << p
        names.append(f"{nplanes} planes, 2^{p} among dense neighbours")
        planes.append(lin)
    # the only one of a segment is its first symbol, and the zero run it ends began in the segment before (the ring
    # before is all zeros as well: nothing of it is significant, its segments have no refinement block to end the run)
    for p in (mid, 0):
        lin = _base(nplanes, 400 + p, quiet_rings=2)
        lin[0, r0] = 1 << p
        names.append(f"{nplanes} planes, 2^{p} first after a boundary that a zero run straddles")
        planes.append(lin)
    streams = []
    for lin in planes:
        data, st = orc.encode_lin(lin, W0, H0)
        assert list(st.planes)[:1] == [nplanes]
        streams.append(data)
    return names, np.stack(planes), streams


@pytest.mark.parametrize("nplanes", [7, 11])
def test_crafted_planes(ctx, opts, nplanes):
    """The streams are the oracle's entropy stage on the planes (and the encoder's: tests/test_pack_gpu.py's way); as one
    batch (one path family, four parts) and each on its own (both families)."""
    import torch

    names, planes, streams = crafted(nplanes)
    got, _ = ctx.encode_planes(torch.from_numpy(planes.reshape(-1, W0 * H0)).cuda(), W0, H0, 1)
    assert got == streams
    both_ways(ctx, opts, streams, W0, H0, 1, whole=planes)
    for i in range(len(streams)):
        both_ways(ctx, opts, streams[i:i + 1], W0, H0, 1, whole=planes[i:i + 1])


@pytest.mark.parametrize("nplanes", [7, 11])
def test_crafted_planes_both_families_from_the_start(ctx, opts, nplanes):
    names, planes, streams = crafted(nplanes)
    opts.set("two_families", 1)
    both_ways(ctx, opts, streams, W0, H0, 1, whole=planes)


@pytest.mark.parametrize("nplanes", [7, 11])
def test_crafted_planes_beside_streams_that_take_the_second_walk(ctx, opts, nplanes):
    """tests/test_pack_gpu.py's parity-locked rings give the one-family walk up: those images are reset (k_part_reset)
    and walked again with both families, the flags of their first walk go with its bits."""
    import dwt_amd
    from test_pack_gpu import _parity_locked_planes

    names, planes, streams = crafted(nplanes)
    locked = [_parity_locked_planes(W0, H0, sign, 0) for sign in (1, -1)]
    lstreams = [orc.encode_lin(lin, W0, H0)[0] for lin in locked]
    batch = streams[:5] + lstreams[:1] + streams[5:9] + lstreams[1:] + streams[9:]
    whole = np.concatenate([planes[:5], locked[0][None], planes[5:9], locked[1][None], planes[9:]])
    both_ways(ctx, opts, batch, W0, H0, 1, whole=whole)
    opts.set("no_second_walk", 1)
    with pytest.raises(dwt_amd.DwtxError):   # (the locked ones really do give up)
        ctx.decode_planes(batch, W0, H0, 1)


@pytest.mark.parametrize("nplanes", [7, 11])
def test_crafted_planes_with_sidecar_indices(ctx, opts, nplanes):
    """A correct index: every segment is walked by a wave of its own (k_tokenize<true>).  A foreign one (the next
    stream's): the indexed walk is turned down and the serial one starts over."""
    import dwt_amd

    names, planes, streams = crafted(nplanes)
    n = len(streams)
    made = ctx.set_index(None, n)
    try:
        both_ways(ctx, opts, streams, W0, H0, 1, whole=planes)
        assert all(made[i].magic == dwt_amd.INDEX_MAGIC and made[i].nsegs > 0 for i in range(n))
        ctx.set_index(made, 0)
        opts.set("no_index_fallback", 1)   # a rejected index would be an error: these are all accepted
        both_ways(ctx, opts, streams, W0, H0, 1, whole=planes)
        opts.set("no_index_fallback", 0)
        foreign = (dwt_amd.Index * n)()
        for i in range(n):
            ctypes.memmove(ctypes.byref(foreign[i]), ctypes.byref(made[(i + 1) % n]), ctypes.sizeof(dwt_amd.Index))
        ctx.set_index(foreign, 0)
        both_ways(ctx, opts, streams, W0, H0, 1, whole=planes)
        opts.set("no_index_fallback", 1)
        with pytest.raises(dwt_amd.DwtxError):   # (they really are turned down)
            ctx.decode_planes(streams, W0, H0, 1)
    finally:
        ctx.set_index()


def test_a_flat_image_beside_others_in_a_batch_of_two_parts(ctx, opts):
    """Four images are two parts; image 1 is flat (plane count 0: its only segments are the "plane -1" ones, no flag
    is ever raised for it), image 2 is not: the flags are per image."""
    names, planes, streams = crafted(7)
    flat, _ = orc.encode(np.full((H0, W0, 1), 90, dtype=np.uint8))
    pic, _ = orc.encode(orc.synth(W0, H0, 1, 46, 0))
    both_ways(ctx, opts, [pic, flat, streams[1], streams[4]], W0, H0, 1)
    opts.set("decode_parts", 2)
    both_ways(ctx, opts, [streams[0], flat, pic, flat], W0, H0, 1)


# ---- cut and damaged streams ---------------------------------------------------------------------------------

def test_cut_and_damaged_streams(ctx, opts):
    """The 256x192 picture's stream cut at 40 seeded lengths, some of them just behind the end of a segment's first
    pass (where its refinement block or the next segment begins), and with one seeded byte flipped in each third."""
    W, H, Cn = 256, 192, 1
    data, _ = orc.encode(orc.synth(W, H, Cn, 42, 0))
    made = ctx.set_index(None, 1)
    try:
        both_ways(ctx, opts, [data], W, H, Cn)
    finally:
        ctx.set_index()
    g = orc.geometry(W, H)
    seg = [made[0].seg[k] for k in range(made[0].nsegs)]
    assert len(seg) > 8
    ends = []   # first-pass ends: the next segment's start less this segment's refinement bits
    for a, b in zip(seg, seg[1:]):
        l, p = (a.desc >> 4) & 15, (a.desc >> 8) - 1
        ring = g.pixels[l + 1] - g.pixels[l]
        ends.append(b.bit - (ring - a.n1 if p >= 0 else 0))
    rng = np.random.default_rng(4042)
    cuts = sorted(int(c) for c in rng.choice(np.arange(7, len(data)), 32, replace=False))
    for k in rng.choice(len(ends), 8, replace=False):
        cuts.append(min(int(ends[k]) // 8 + 1 + int(rng.integers(0, 2)), len(data) - 1))
    assert len(cuts) == 40
    both_ways(ctx, opts, [data[:c] for c in cuts], W, H, Cn)
    damaged = []
    for third in range(3):
        lo, hi = max(6, third * len(data) // 3), (third + 1) * len(data) // 3
        for _ in range(4):
            b = bytearray(data)
            b[int(rng.integers(lo, hi))] ^= int(rng.integers(1, 256))
            damaged.append(bytes(b))
    both_ways(ctx, opts, damaged, W, H, Cn)
