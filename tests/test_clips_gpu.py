"""GPU: clip stacks — dwtx_encode_view_clips / dwtx_decode_view_clips (include/dwtx.h): one stack whose every period-th window is
a key coded as itself, every other window a link coded against the window before it; many clips per call.

The decode is stated by equivalence, and both sides of it are yardsticks here: the oracle's fold on the CPU (tests/clips.py) and
the loop a caller had to write before — a plain decode_view per whole key, a decode_view(..., base=window before) per link, one
stream each — bit for bit, host_info included.  Every destination is prefilled with seeded random samples of the range, so that
a base taken from the wrong place changes the result, and every comparison covers the WHOLE destination buffer, padding and gaps
included.  Layouts are tests/test_chain_gpu.py's DESTS with 11 windows (the tile grid one column off the quad has 3 x 4: 11 is
no product, and a band of 11 tiles stands for the grid on the quad); shapes are tests/signed.py's and nothing larger."""
import itertools

import numpy as np
import pytest

import chain
import clips
import delta
import history
import levels
import orc
import test_chain_gpu as CG
import test_delta_gpu as G
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
SHAPES = delta.SHAPES
KINDS = G.KINDS
KIND_NAMES = G.KIND_NAMES
N = 11
PERIODS = (1, 4, 5, 11)     # segments of 1 to 11 windows meet lift.hip's CHAIN_AHEAD = 4 at every remainder; the last clip is one picture

assert set(CG.DESTS) == {"dense", "stack", "tiles", "off1", "planar", "step"}
DESTS = {   # test_chain_gpu.DESTS, each with N windows: name -> (Layout, stepped)
    "dense": lambda W, H, Cn: (G.dense(W, H, Cn, N), False),
    "stack": lambda W, H, Cn: (V.stack(W, H, Cn, N), False),
    "tiles": lambda W, H, Cn: (V.grid(W, H, Cn, "quad", rows=1, cols=N), False),
    "off1": lambda W, H, Cn: (V.grid(W, H, Cn, "off1", rows=3, cols=4), False),      # (12 windows)
    "planar": lambda W, H, Cn: (G.nchw(W, H, N), False),
    "step": lambda W, H, Cn: (G.stepped(W, H, Cn, 4 if Cn == 3 else 2, N), True),
}
CASES = [(wh, Cn, dest) for wh in SHAPES for Cn in (1, 3) for dest in DESTS if Cn == 3 or dest != "planar"]
_case_id = lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], "gray" if c[1] == 1 else "rgb", c[2])   # noqa: E731


def kind_of(case):
    """Every destination meets the three sample types over the shapes and the channel counts."""
    (W, H), Cn, dest = case
    return KIND_NAMES[(SHAPES.index((W, H)) + list(DESTS).index(dest) + Cn) % 3]


def test_the_cases_cover_every_sample_type():
    seen = {(Cn, dest, kind_of((wh, Cn, dest))) for wh, Cn, dest in CASES}
    assert len(seen) == 3 * 11


# ---- the rows of a decode ------------------------------------------------------------------------------------------------------

def sweep_rows(W, H, Cn, kind, n, period):
    """n streams of a stack of successor frames under `period`, every one readable to its finest level: every third link replaced
    by a cut residual of the block pictures (delta.cut_fixture, 0.6 and 0.33 in turn: every clamp of a link acts and the clip goes
    on from clamped samples), the last key by the cut block picture (clips.cut_key: the plain pictures' clamps act)."""
    lo, hi = KINDS[kind][:2]
    datas = clips.streams(clips.frames(W, H, Cn, lo, hi, n), period)
    links = [i for i in range(n) if not clips.is_key(i, period)]
    for i, cut in zip(links[1::3], itertools.cycle(delta.CUTS[::-1])):
        datas[i] = delta.cut_fixture(W, H, Cn, lo, hi, cut)[0]
    datas[(n - 1) // period * period] = clips.cut_key(W, H, Cn, lo, hi)[0]
    return datas


_folds = {}


def oracle(datas, initial, period, W, H, Cn, lo, hi, independent=False):
    """clips.decode, made once.  independent: every stream is readable to its finest level, so no window keeps what lay there and
    the fold is shared by every layout and prefill."""
    k = (tuple(datas), None if independent else tuple(w.tobytes() for w in initial), period, W, H, Cn, lo, hi)
    if k not in _folds:
        _folds[k] = clips.decode(datas, initial, period, W, H, Cn, lo, hi)
        assert not independent or not any(r is None or r is clips.UNTOUCHED for r in _folds[k][1])
    return _folds[k]


class Run:
    """One clips decode's buffers: the destination (prefilled), on the host and on the device."""

    def __init__(self, c, kind, Ld, order="rgb", seed=0):
        lo, hi, dt, sgn = KINDS[kind] if isinstance(kind, str) else kind
        self.c, self.kind, self.Ld, self.order = c, kind, Ld, order
        self.lo, self.hi, self.dt, self.sgn = lo, hi, dt, sgn
        self.buf = CG.prefill(Ld.samples, kind, seed)
        self.initial = [G.in_memory(w, order).copy() for w in Ld.np_windows(self.buf)]   # (as pictures: R, G, B)
        self.tbuf = V.to_device(c, self.buf)

    def keywords(self, stepped):
        return dict(maxval=self.hi, stepped=stepped, order=self.order, signed=self.sgn, minval=self.lo if self.sgn else None)

    def clips(self, streams, lens, period, stepped=False):
        return self.c.decode_view_clips(streams, lens, self.Ld.t_view(self.tbuf), period, **self.keywords(stepped))

    def loop(self, streams, lens, period, stepped=False):
        """What a caller writes without the clips call, window by window: a key's stream through the plain decode_view — into a
        window of its own first, which says whether it is whole, and only then into its place: a cut key's corner is the one
        thing the clips call does not write —, a link's through decode_view(base=the window before).  The tiles of a grid's band
        lie side by side: their spans meet, which the delta call refuses though no sample is shared, so the base is a copy there."""
        import torch

        infos = []
        beside = len(self.Ld.shape) == 5
        H, W = self.Ld.shape[-3:-1]
        T = orc.geometry(W, H).levels
        for i in range(self.Ld.n):
            one, here = (streams[i:i + 1], lens[i:i + 1]), CG.window_view(self.Ld, self.tbuf, i)
            if clips.is_key(i, period):
                aside = torch.zeros(tuple(here.shape), dtype=here.dtype, device=here.device)
                I = self.c.decode_view(*one, aside, **dict(self.keywords(False), order=self.order))
                if I[0].status == 0 and I[0].level == T - 1:
                    I = self.c.decode_view(*one, here, **self.keywords(stepped))
                infos += I
            else:
                base = CG.window_view(self.Ld, self.tbuf, i - 1)
                infos += self.c.decode_view(*one, here, base=base.clone() if beside else base, **self.keywords(stepped))
        return infos

    def got(self):
        return V.to_host(self.tbuf, self.dt == np.uint16)

    def check_against_oracle(self, datas, period, infos, independent=False):
        H, W, Cn = self.initial[0].shape
        windows, results = oracle(datas, self.initial, period, W, H, Cn, self.lo, self.hi, independent)
        want = self.buf.copy()
        for w, pic in zip(self.Ld.np_windows(want), windows):
            w[...] = G.in_memory(pic, self.order)
        T = orc.geometry(W, H).levels
        for i, (ref, I) in enumerate(zip(results, infos)):
            if ref is None:
                assert I.status != 0, i
            else:
                assert I.status == 0 and (I.level == T - 1) == (ref is not clips.UNTOUCHED), (i, I.status, I.level)
        got = self.got()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (period, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
        return results


def both_ways(c, kind, Ld, datas, period, stepped=False, order="rgb", seed=0, independent=False):
    """The clips call against the oracle's fold, then the loop of existing calls on a second buffer with the same prefill against
    the clips call's buffer, bit for bit, with the same host_info.  -> the clips call's infos and the oracle's results."""
    streams, lens = G.to_streams(c, datas)
    a = Run(c, kind, Ld, order, seed)
    infos = a.clips(streams, lens, period, stepped)
    results = a.check_against_oracle(datas, period, infos, independent)
    b = Run(c, kind, Ld, order, seed)
    infos_b = b.loop(streams, lens, period, stepped)
    ga, gb = a.got(), b.got()
    bad = np.flatnonzero(ga != gb)
    assert bad.size == 0, (period, bad.size, bad[:8])
    assert [CG.info_fields(I) for I in infos] == [CG.info_fields(I) for I in infos_b], period
    return infos, results


# ---- decode: every layout under every period -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_clips_decode_equals_the_fold_and_the_loop_of_existing_calls(ctx, case):
    """1: every destination layout, all three sample types, gray and RGB, periods 1, 4, 5 and 11 (one clip; 12 windows: one more)."""
    (W, H), Cn, dest = case
    kind = kind_of(case)
    Ld, stp = DESTS[dest](W, H, Cn)
    for period in PERIODS:
        datas = sweep_rows(W, H, Cn, kind, Ld.n, period)
        both_ways(ctx, kind, Ld, datas, period, stepped=stp, seed=period, independent=True)


def whole_rows(W, H, Cn, kind, n, period):
    """n whole streams: every host_info of the batch is the same, so the decoder finishes each of its parts as ONE group and
    lift.hip's k_clips_from_planes gets launches of several windows and several segments — a batch with one cut stream in a part
    falls back to a launch per window (codec.hip, decode_device's `part`), which is all that sweep_rows ever gives the kernel."""
    lo, hi = KINDS[kind][:2]
    return clips.streams(clips.frames(W, H, Cn, lo, hi, n), period)


UNIFORM = [("one_stream", 1), None]   # one group of all 11 windows; the two parts [0,5) [5,11), the second starting mid-clip


@pytest.mark.parametrize("switch", UNIFORM, ids=["one-group", "two-parts"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_whole_streams_walk_segments_of_several_windows(ctx, opts, case, switch):
    """1: the layouts and periods of the sweep above with whole streams.  One group: segments of 1 | 4, 4, 3 | 5, 5, 1 | 11 windows
    (12 windows: 4, 4, 4 | 5, 5, 2 | 11, 1) side by side in one launch, with second and third batches of CHAIN_AHEAD pictures, the
    prefetch behind a full batch and a tail of every remainder.  Two parts: [5,11) starts 1, 0 and 5 windows into a clip, its
    first segment (3, none and 6 windows) takes window 4 as it lies in memory."""
    (W, H), Cn, dest = case
    kind = kind_of(case)
    Ld, stp = DESTS[dest](W, H, Cn)
    if switch:
        opts.set(*switch)
    for period in PERIODS:
        both_ways(ctx, kind, Ld, whole_rows(W, H, Cn, kind, Ld.n, period), period, stepped=stp, seed=20 + period, independent=True)


@pytest.mark.parametrize("Cn,kind", [(1, "s16"), (3, "u8"), (3, "u16")], ids=["gray-s16", "rgb-u8", "rgb-u16"])
def test_segments_of_every_length_in_one_launch(ctx, opts, Cn, kind):
    """1: one group of 11 windows under every period from 1 to 11: segments of every length from 1 to 11, and every length of a
    last, shorter one."""
    W, H = 132, 72
    opts.set("one_stream", 1)
    for period in range(1, N + 1):
        both_ways(ctx, kind, V.stack(W, H, Cn, N), whole_rows(W, H, Cn, kind, N, period), period, seed=40 + period, independent=True)


@pytest.mark.parametrize("dest", ["dense", "planar", "step", "tiles"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_clips_decode_of_bgr_pixels(ctx, wh, dest):
    W, H = wh
    kind = KIND_NAMES[(SHAPES.index(wh) + len(dest)) % 3]
    Ld, stp = DESTS[dest](W, H, 3)
    for period in (4, 11):
        both_ways(ctx, kind, Ld, sweep_rows(W, H, 3, kind, Ld.n, period), period, stepped=stp, order="bgr", seed=3, independent=True)


# ---- decode: a mixed batch under the switches --------------------------------------------------------------------------------------

def mixed_rows(W, H, Cn, kind):
    """11 windows, period 4 — keys 0, 4 and 8: key cut before its finest level, link, link cut at 0.6 (clamped, whole), link |
    unreadable key, link, link cut before its finest level, link | key cut at a third of its length, link, unreadable link.
    Clips 0 and 1 are built on the prefill of windows 0 and 4, which stay; window 6 stays and window 7 goes on from it.
    The key cut at a third: these streams are progressive by bit plane, every level from the first planes on, and a third of
    a key's length still reaches the finest level for every shape, range and picture tried (successor frames, noise, blocks) —
    so by the contract that key IS written, from the planes it has, and the links behind it build on that; the key whose window
    stays is the one cut before its finest level, window 0.  Both are held to the fold."""
    lo, hi = KINDS[kind][:2]
    datas = clips.streams(clips.frames(W, H, Cn, lo, hi, N), 4)
    datas[0] = levels.late_prefix(datas[0], W, H, Cn, orc.geometry(W, H).levels - 2)
    datas[2] = delta.cut_fixture(W, H, Cn, lo, hi, 0.6)[0]
    datas[4] = b"\xff\xff" + datas[4][2:]
    datas[6] = levels.late_prefix(datas[6], W, H, Cn, orc.geometry(W, H).levels - 2)
    datas[8] = datas[8][:len(datas[8]) // 3]
    datas[10] = b"\xff\xff" + datas[10][2:]
    return datas


@pytest.mark.parametrize("switch", CG.SWITCHES, ids=lambda s: "plain" if s is None else "%s=%d" % s)
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_a_mixed_batch_under_the_switches(ctx, opts, wh, switch):
    """2: decode_parts 2 and 4 cut the clips mid-segment ([0,5) [5,11); [0,2) [2,5) [5,8) [8,11)) and the per-image fallback runs;
    windows that stay are the next links' bases, keys included."""
    W, H = wh
    if switch:
        opts.set(*switch)
    for Cn, kind, dest in ((1, KIND_NAMES[SHAPES.index(wh)], "stack"), (3, KIND_NAMES[(SHAPES.index(wh) + 1) % 3], "planar")):
        Ld = DESTS[dest](W, H, Cn)[0]
        datas = mixed_rows(W, H, Cn, kind)
        infos, results = both_ways(ctx, kind, Ld, datas, 4, seed=4)
        assert [i for i, x in enumerate(results) if x is None] == [4, 10]
        assert [i for i, x in enumerate(results) if x is clips.UNTOUCHED] == [0, 6]
        T = orc.geometry(W, H).levels
        assert infos[4].status != 0 and infos[10].status != 0 and infos[0].level == T - 2 and infos[6].level == T - 2
        assert infos[8].status == 0 and infos[8].level == T - 1
        assert (results[8] != clips.frames(W, H, Cn, *KINDS[kind][:2], N)[8]).any()   # (whole in size, not in planes)


# ---- decode: the clamp fixture ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_the_clamp_fixture(ctx, wh, Cn, kind):
    """3: two clips of five — the four cut links of chain.clamp_fixture behind their key, a block picture of the range: whole in
    clip 0, cut at 0.6 of its length in clip 1, where the finest level is still reached and the key's own clamps act on at least
    10 % of the samples at each end (tests/test_clips_cpu.py holds the cut to that; 0.6 reaches it for every shape and range, so no
    other cut of delta.CUTS is needed)."""
    W, H = wh
    lo, hi = KINDS[kind][:2]
    key, links, _ = chain.clamp_fixture(W, H, Cn, lo, hi)
    cut, pic = clips.cut_key(W, H, Cn, lo, hi)
    assert (pic == key).all()
    datas = [clips.plain_stream(key)[0]] + links + [cut] + links
    Ld = G.dense(W, H, Cn, 10) if Cn == 1 else V.stack(W, H, Cn, 10)
    _, results = both_ways(ctx, kind, Ld, datas, 5, seed=5, independent=True)
    assert (results[0] == key).all() and (results[5] != key).any()
    assert any((a != b).any() for a, b in zip(results[1:5], results[6:]))


# ---- encode ------------------------------------------------------------------------------------------------------------------------

def encode_pairs(fr, period):
    """The stack as (picture, base) pairs for G.check_streams: a key against a picture of zeros, whose residual is the key itself —
    the oracle's stream of that residual IS the plain stream of the key, which is asserted here."""
    zero = np.zeros_like(fr[0])
    prs = [(f, zero if clips.is_key(i, period) else fr[i - 1]) for i, f in enumerate(fr)]
    for i, (S, B) in enumerate(prs):
        if B is zero:
            assert delta.stream(S, B)[0] == clips.plain_stream(S)[0], i
    return prs


@pytest.mark.parametrize("case", [c for c in CASES if c[2] in ("dense", "off1", "planar", "step")], ids=_case_id)
def test_clips_encode_equals_the_oracle_and_the_existing_calls(ctx, case):
    """4: streams and records equal the oracle's (plain streams for keys, residual streams for links) and, window by window, the
    plain encode of a key and the delta encode of a link, byte for byte, whole buffers, with and without a capacity of 500."""
    import torch

    (W, H), Cn, dest = case
    kind = kind_of(case)
    lo, hi, dt, sgn = KINDS[kind]
    Ls, stp = DESTS[dest](W, H, Cn)
    n, period = Ls.n, 4
    fr = list(clips.frames(W, H, Cn, lo, hi, n))
    fr[5] = delta.clamp_pair(W, H, Cn, lo, hi)[0]   # (one block picture: residuals of the whole range around it)
    bufS, tS = G.load(ctx, Ls, fr, dt)
    src = Ls.t_view(tS)
    stride = ctx.lib.dwtx_encode_bound16(W, H, Cn)
    for capacity in (0, 500):
        shape = (n, stride if capacity <= 0 else (capacity + 15) // 8 * 8)
        out = torch.full(shape, G.FILL, dtype=torch.uint8, device=ctx.device)
        out, info = ctx.encode_view_clips(src, period, capacity, out=out, stepped=stp, signed=sgn)
        G.check_streams(out, info, encode_pairs(fr, period), capacity)
        each, each_info = torch.full(shape, G.FILL, dtype=torch.uint8, device=ctx.device), torch.zeros_like(info)
        for i in range(n):
            base = None if clips.is_key(i, period) else CG.window_view(Ls, tS, i - 1)
            ctx.encode_view(CG.window_view(Ls, tS, i), capacity, out=each[i:i + 1], info=each_info[i:i + 1], stepped=stp, signed=sgn, base=base)
        assert torch.equal(out, each)
        assert [V.fields(I) for I in V.infos_of(info)] == [V.fields(I) for I in V.infos_of(each_info)]
    assert (V.to_host(tS, dt == np.uint16) == bufS).all(), "the source was written to"


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_clips_encode_in_parts_that_start_mid_clip(ctx, order):
    """4: 133 windows run as four parts of the encoder, which start at windows 33, 66 and 99 — inside a clip of period 5: each
    part's first link reads the window before the part.  Against one plain encode and one delta encode of the whole stack."""
    import torch

    W, H, Cn, n, period = 132, 72, 3, 133, 5
    fr = clips.frames(W, H, Cn, 0, 255, 12)
    t = V.to_device(ctx, np.stack([fr[(i * 7) % 12] for i in range(n)]))
    out, info = ctx.encode_view_clips(t, period, order=order)
    plain, pinfo = ctx.encode_view(t, order=order)
    links, linfo = ctx.encode_view(t[1:], base=t[:-1], order=order)
    lens = ctx.stream_lengths(info)
    pl, ll = ctx.stream_lengths(pinfo), ctx.stream_lengths(linfo)
    got, fp, fl = V.infos_of(info), V.infos_of(pinfo), V.infos_of(linfo)
    for i in range(n):
        key = clips.is_key(i, period)
        k = int(pl[i]) if key else int(ll[i - 1])
        assert int(lens[i]) == k, i
        assert torch.equal(out[i, :k], plain[i, :k] if key else links[i - 1, :k]), i
        assert V.fields(got[i]) == V.fields(fp[i] if key else fl[i - 1]), i


BIG = {   # 128 windows or more: the encoder runs four parts; name -> (Layout, stepped, kind)
    "grid": lambda W, H, Cn: (V.grid(W, H, Cn, "off1", rows=11, cols=12), False, "u16"),     # (parts move the grid's `first`)
    "planar": lambda W, H, Cn: (G.nchw(W, H, 133), False, "s16"),
    "step": lambda W, H, Cn: (G.stepped(W, H, Cn, 4, 133), True, "u8"),
}


@pytest.mark.parametrize("dest", list(BIG))
def test_clips_encode_in_parts_of_a_grid_planar_and_stepped_view(ctx, dest):
    """4: the part boundaries inside a clip where a part's view is not a moved pointer: a tile grid of 11 x 12 (parts at windows
    33, 66 and 99, mid-band and mid-clip under period 5: the window before a part is window first - 1 of the grid), planar and
    stepped stacks of 133 (the same boundaries).  Window by window against the plain encode of a key and the delta encode of a link."""
    import torch

    W, H, Cn, period = 132, 72, 3, 5
    Ls, stp, kind = BIG[dest](W, H, Cn)
    lo, hi, dt, sgn = KINDS[kind]
    n = Ls.n
    assert n >= 128 and all((n * k // 4) % period for k in (1, 2, 3))
    some = clips.frames(W, H, Cn, lo, hi, 12)
    fr = [some[(i * 7) % 12] for i in range(n)]
    bufS, tS = G.load(ctx, Ls, fr, dt)
    out, info = ctx.encode_view_clips(Ls.t_view(tS), period, stepped=stp, signed=sgn)
    each, each_info = torch.zeros_like(out), torch.zeros_like(info)
    for i in range(n):
        base = None if clips.is_key(i, period) else CG.window_view(Ls, tS, i - 1)
        ctx.encode_view(CG.window_view(Ls, tS, i), out=each[i:i + 1], info=each_info[i:i + 1], stepped=stp, signed=sgn, base=base)
    got, want = V.infos_of(info), V.infos_of(each_info)
    for i in range(n):
        assert V.fields(got[i]) == V.fields(want[i]), i
        k = got[i].nbytes
        assert torch.equal(out[i, :k], each[i, :k]), i
    assert (V.to_host(tS, dt == np.uint16) == bufS).all(), "the source was written to"


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_the_encode_index_lands_at_entry_i_and_the_decode_takes_it(ctx, opts, Cn):
    """4: the index of stream i at entry i, a key's and a link's alike; the clips decode is offered them with no_index_fallback
    set (an index that is turned down is then an error)."""
    import torch

    import dwt_amd

    W, H, n, period, kind = 132, 72, 7, 3, "u8"
    lo, hi, dt, sgn = KINDS[kind]
    fr = clips.frames(W, H, Cn, lo, hi, n)
    t = V.to_device(ctx, np.stack(fr))
    dev_index = ctx.set_encode_index(n, device=True)
    try:
        out, info = ctx.encode_view_clips(t, period)
        enc = [dwt_amd.index_from_row(dev_index[i]) for i in range(n)]
    finally:
        ctx.set_encode_index()
    assert all(X.magic == dwt_amd.INDEX_MAGIC and X.nsegs > 0 and (X.W, X.H, X.C) == (W, H, Cn) for X in enc)
    lens = ctx.stream_lengths(info)
    alone = []
    for i in range(n):   # each stream's own index, from an encode of it alone
        one = ctx.set_encode_index(1, device=True)
        try:
            ctx.encode_view(t[i:i + 1], base=None if clips.is_key(i, period) else t[i - 1:i])
            alone.append(dwt_amd.index_from_row(one[0]))
        finally:
            ctx.set_encode_index()

    def index_fields(X):   # (an encode writes an entry's header and seg[:nsegs], nothing behind them)
        return (X.magic, X.W, X.H, X.C, X.nsegs, X.stream_bits, [(s.bit, s.sym_base, s.n1, s.cnt, s.desc, s.order) for s in X.seg[:X.nsegs]])

    assert len({X.stream_bits for X in enc}) == n   # (seven streams of seven lengths: an entry in the wrong place shows)
    assert [index_fields(X) for X in enc] == [index_fields(X) for X in alone]
    back = V.to_device(ctx, CG.prefill(t.numel(), kind, 9).reshape(t.shape))
    opts.set("no_index_fallback", 1)
    ctx.set_index((dwt_amd.Index * n)(*enc), 0)
    try:
        infos = ctx.decode_view_clips(out, lens, back, period)
    finally:
        ctx.set_index()
    assert [I.status for I in infos] == [0] * n and torch.equal(back, t)


@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_round_trip_of_a_stack(ctx, wh, Cn, kind):
    """5: encode_view_clips, then decode_view_clips into random samples; periods 3 (three clips, the last short) and n (one clip)."""
    import torch

    W, H = wh
    n = 8
    lo, hi, dt, sgn = KINDS[kind]
    fr = clips.frames(W, H, Cn, lo, hi, n)
    t = V.to_device(ctx, np.stack(fr))
    for period in (3, n):
        out, info = ctx.encode_view_clips(t, period, signed=sgn)
        assert all(I.error == 0 for I in V.infos_of(info))
        back = V.to_device(ctx, CG.prefill(t.numel(), kind, 7).reshape(t.shape))
        infos = ctx.decode_view_clips(out, ctx.stream_lengths(info), back, period, maxval=hi, signed=sgn, minval=lo if sgn else None)
        assert [I.status for I in infos] == [0] * n
        assert torch.equal(back, t) and (V.to_host(t, dt == np.uint16) == np.stack(fr)).all()


@pytest.mark.parametrize("sgn", [0, 1], ids=["uint16", "int16"])
def test_round_trip_of_a_full_range_stack(ctx, sgn):
    """5: frames over the whole range of the type, whose residuals leave int16; the keys are full-range pictures coded as they are."""
    import torch

    W, H, n, period = 132, 72, 6, 3
    kind = (-32768, 32767, np.int16, True) if sgn else (0, 65535, np.uint16, False)
    fr = chain.full_range_frames(W, H, sgn, n - 1)
    assert all(delta.residual(fr[i], fr[i - 1]).min() < -32768 or delta.residual(fr[i], fr[i - 1]).max() > 32767 for i in (1, 2, 4, 5))
    t = V.to_device(ctx, np.stack(fr))
    out, info = ctx.encode_view_clips(t, period, signed=bool(sgn))
    G.check_streams(out, info, encode_pairs(fr, period), prefilled=False)
    back = V.to_device(ctx, CG.prefill(t.numel(), kind, 8).reshape(t.shape))
    infos = ctx.decode_view_clips(out, ctx.stream_lengths(info), back, period, maxval=kind[1], signed=bool(sgn), minval=kind[0] if sgn else None)
    assert [I.status for I in infos] == [0] * n and torch.equal(back, t)


def test_a_picture_of_more_than_16_planes_is_refused_alone(ctx):
    """4: the residual of two full-range noise pictures needs 18 planes: error = 1 for that link, the others of the batch are coded."""
    W, H = 132, 72
    a, b = delta.noise_pair(W, H, 0)
    fr = chain.full_range_frames(W, H, 0, 2) + [a, b]
    t = V.to_device(ctx, np.stack(fr))
    out, info = ctx.encode_view_clips(t, 5)
    errors = [I.error for I in V.infos_of(info)]
    assert errors[4] == 1 and errors[:3] == [0, 0, 0], errors
    G.check_streams(out, info, encode_pairs(fr, 5)[:3], prefilled=False)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_with_their_texts_and_nothing_written(ctx):
    """6"""
    import torch

    import dwt_amd

    W, H, n = 132, 72, 4
    t = torch.full((n, H, W, 1), 7, dtype=torch.uint8, device=ctx.device)
    streams = torch.zeros((n, 4096), dtype=torch.uint8, device=ctx.device)
    lens = torch.full((n,), 100, dtype=torch.int64, device=ctx.device)
    out = torch.full((n, 4096), 3, dtype=torch.uint8, device=ctx.device)
    lib, Cc = ctx.lib, dwt_amd.C
    v, vW, vH, Cn, vn, step = ctx._view(t, 255)
    infos = (dwt_amd.DecodeInfo * n)()
    info = torch.zeros((n, Cc.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)

    def c_decode(view, period, sgn=0, minval=0):
        return lib.dwtx_decode_view_clips(ctx.h, streams.data_ptr(), streams.shape[1], lens.data_ptr(), W, H, n, view, step, period, 0, sgn, minval,
                                          Cc.cast(infos, Cc.c_void_p))

    def c_encode(view, period, sgn=0, minval=0):
        return lib.dwtx_encode_view_clips(ctx.h, view, step, period, 0, sgn, W, H, n, 0, out.data_ptr(), out.shape[1], info.data_ptr())

    def view(**changes):
        f = dict(dev=t.data_ptr(), sample_bytes=1, channels=1, maxval=255, cols=0, row_pitch=W, image_stride=H * W, band_stride=0, channel_stride=0)
        f.update(changes)
        return Cc.byref(dwt_amd.View(f["dev"], f["sample_bytes"], f["channels"], f["maxval"], f["cols"], f["row_pitch"], f["image_stride"],
                                     f["band_stride"], f["channel_stride"]))

    def text():
        return lib.dwtx_last_error().decode()

    for call in (c_decode, c_encode):
        for period in (0, -3):
            assert call(Cc.byref(v), period) == ERR_ARG and text().startswith("clips view: period %d" % period), text()
        assert call(None, 2) == ERR_ARG and text().startswith("clips view: no view"), text()
        assert call(Cc.byref(v), 2, sgn=1) == ERR_ARG and text().startswith("clips view:") and "int16_t" in text(), text()
        assert call(view(dev=None), 2) == ERR_ARG and text().startswith("clips view:"), text()
        assert call(view(row_pitch=W - 1), 2) == ERR_ARG and text().startswith("clips view: row_pitch"), text()
        assert call(view(channels=2), 2) == ERR_ARG and text().startswith("clips view:") and "channels 2" in text(), text()
    assert c_decode(view(sample_bytes=2, row_pitch=W // 2, image_stride=H * W // 2, maxval=4095), 2, sgn=0, minval=-5) == ERR_ARG
    assert text().startswith("clips view: minval -5 without sgn"), text()
    assert c_decode(view(maxval=100), 2) == ERR_ARG and text().startswith("clips view: maxval 100"), text()
    assert c_decode(view(image_stride=H * W - W), 2) == ERR_ARG and text().startswith("clips view: windows overlap"), text()
    s16 = torch.zeros((n, H, W, 1), dtype=torch.int16, device=ctx.device)
    with pytest.raises(dwt_amd.DwtxError) as e:
        ctx.decode_view_clips(streams, lens, s16, 2, signed=True, minval=50, maxval=10)
    assert e.value.rc == ERR_ARG and "clips view:" in str(e.value) and "minval < maxval" in str(e.value), str(e.value)
    assert (t == 7).all() and not s16.any() and (out == 3).all() and not info.any()
    # in Python, before any device call: the keywords of the other view calls, a key outside the stack, lists, floats, no period
    bad = [dict(period=2, flip="y"), dict(period=2, levels_max=2), dict(period=2, crop=(64, 64)), dict(period=2, base=t), dict(period=2, key=t[0]),
           dict(period=2, windows=[t[0]]), dict(period=0), dict(period=-1), dict(period=2.5), dict(period=None), dict(period=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.decode_view_clips(streams, lens, t, **kw)
        if "levels_max" not in kw and "crop" not in kw:
            with pytest.raises(ValueError):
                ctx.encode_view_clips(t, **kw)
    for into in (t.float(), [t[0], t[1], t[2], t[3]]):
        with pytest.raises(ValueError):
            ctx.decode_view_clips(streams, lens, into, 2)
        with pytest.raises(ValueError):
            ctx.encode_view_clips(into, 2)
    assert (t == 7).all() and (out == 3).all()


# ---- the context's history ---------------------------------------------------------------------------------------------------------

@pytest.fixture
def fresh(ctx):
    """A context that has run nothing yet (it depends on `ctx`: no GPU, no test)"""
    import dwt_amd

    c = dwt_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("Cn,kind", [(1, "s16"), (3, "u8")], ids=["gray-s16", "rgb-u8"])
def test_a_clips_call_after_calls_of_another_geometry_channel_count_and_depth(fresh, Cn, kind):
    """7: tests/history.py's dirt — noise of more planes, at least as large in every dimension a slot is sized by — of the other
    channel count, a transposed geometry and 16-bit depth on a private context, then the clips call, whole result compared."""
    W, H = 263, 135
    datas = mixed_rows(W, H, Cn, kind)
    stride = history.stride_of(datas)
    for cl in (history.call("decode", W, H, 3, n=12, stride=stride), history.call("decode16", H + 1, W + 1, 4 - Cn, n=12, stride=stride),
               history.call("decode", W, H, Cn, n=12, stride=stride), history.call("encode", W, H, Cn, n=12)):
        history.dirty(fresh, cl.W, cl.H, cl.Cn, cl.n, cl.how, cl.kind, cl.stride)
    both_ways(fresh, kind, V.stack(W, H, Cn, N), datas, 4, seed=10)


@pytest.mark.parametrize("Cn,kind", [(1, "u16"), (3, "s16")], ids=["gray-u16", "rgb-s16"])
def test_a_clips_call_as_a_contexts_first_call(fresh, Cn, kind):
    """7"""
    W, H = 263, 135
    datas = mixed_rows(W, H, Cn, kind)
    streams, lens = G.to_streams(fresh, datas)
    r = Run(fresh, kind, V.stack(W, H, Cn, N), seed=11)
    r.check_against_oracle(datas, 4, r.clips(streams, lens, 4))


@pytest.mark.parametrize("Cn,kind", [(1, "u8"), (3, "u16")], ids=["gray-u8", "rgb-u16"])
def test_a_clips_encode_as_a_contexts_first_call(fresh, Cn, kind):
    """7"""
    W, H, n, period = 263, 135, 5, 2
    lo, hi, dt, sgn = KINDS[kind]
    fr = clips.frames(W, H, Cn, lo, hi, n)
    out, info = fresh.encode_view_clips(V.to_device(fresh, np.stack(fr)), period, signed=sgn)
    G.check_streams(out, info, encode_pairs(fr, period), prefilled=False)
