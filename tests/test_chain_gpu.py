"""GPU: delta chains — dwtx_encode_view_chain / dwtx_decode_view_chain (include/dwtx.h): every picture coded against the one
before it, the first against a key, in one call.

The contract is stated by equivalence, and both sides of it are yardsticks here: the oracle's fold on the CPU (tests/chain.py
over tests/delta.py) and the loop a caller had to write before — n calls of decode_view(..., base=previous window) of one
stream each —, bit for bit, host_info included.  Every destination is prefilled with seeded random samples of the range, not a
constant, so that a base taken from the wrong place changes the result, and every comparison covers the WHOLE destination
buffer and the WHOLE key buffer, padding and gaps included.  Layouts are flat buffers plus an offset, a shape and strides, as in
tests/test_views_gpu.py; n is 5 to 7."""
import numpy as np
import pytest

import chain
import delta
import history
import levels
import orc
import test_delta_gpu as G
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
SHAPES = delta.SHAPES
KINDS = G.KINDS
KIND_NAMES = G.KIND_NAMES


# ---- layouts: the destination's (tests/test_delta_gpu.py LAYOUTS' destination sides, with more windows) and the key's ----------

def pitched_key(W, H, Cn):
    """one window off the quad: an odd first sample and an odd pitch"""
    pitch = W * Cn + 3
    return V.Layout(1 + H * pitch + 6, 1, (1, H, W, Cn), (H * pitch, pitch, Cn, 1))


DESTS = {   # name -> (Layout, stepped)
    "dense": lambda W, H, Cn: (G.dense(W, H, Cn, 5), False),
    "stack": lambda W, H, Cn: (V.stack(W, H, Cn, 5), False),                                   # a pitch gap of five samples
    "tiles": lambda W, H, Cn: (V.grid(W, H, Cn, "quad", rows=2, cols=3), False),               # windows of a tile grid, on the quad
    "off1": lambda W, H, Cn: (V.grid(W, H, Cn, "off1", rows=3, cols=2), False),                # one column off it
    "planar": lambda W, H, Cn: (G.nchw(W, H, 7), False),                                       # (RGB only)
    "step": lambda W, H, Cn: (G.stepped(W, H, Cn, 4 if Cn == 3 else 2, 5), True),
}
KEYS = {
    "dense": lambda W, H, Cn: (G.dense(W, H, Cn, 1), False),
    "pitched": lambda W, H, Cn: (pitched_key(W, H, Cn), False),
    "planar": lambda W, H, Cn: (G.nchw(W, H, 1, off=4), False),
    "step": lambda W, H, Cn: (G.stepped(W, H, Cn, 5 if Cn == 3 else 3, 1), True),
}
CASES = [(wh, Cn, dest) for wh in SHAPES for Cn in (1, 3) for dest in DESTS if Cn == 3 or dest != "planar"]
_case_id = lambda c: "%dx%d-%s-%s" % (c[0][0], c[0][1], "gray" if c[1] == 1 else "rgb", c[2])   # noqa: E731


def key_and_kind(case):
    """Every destination meets every key and the three sample types over the shapes and the channel counts."""
    (W, H), Cn, dest = case
    keys = [k for k in KEYS if Cn == 3 or k != "planar"]
    d = list(DESTS).index(dest)
    return keys[(d + Cn) % len(keys)], KIND_NAMES[(SHAPES.index((W, H)) + d + Cn) % 3]


def test_the_cases_cover_every_key_and_sample_type():
    seen = {(Cn, *key_and_kind((wh, Cn, dest))) for wh, Cn, dest in CASES}
    assert {(1, k, s) for k in ("dense", "pitched", "step") for s in KIND_NAMES} <= seen
    assert {k for Cn, k, _ in seen if Cn == 3} == set(KEYS) and {s for Cn, _, s in seen if Cn == 3} == set(KIND_NAMES)


def prefill(samples, kind, seed):
    """Seeded random samples of the range, all over the buffer."""
    lo, hi, dt, _ = KINDS[kind] if isinstance(kind, str) else kind
    return np.random.default_rng(4000 + seed).integers(lo, hi + 1, samples).astype(dt)


# ---- the rows of a decode ------------------------------------------------------------------------------------------------------

def chain_rows(W, H, Cn, kind, n):
    """-> (key picture, n residual streams): a run of successor frames, links 1 and 3 replaced by the cut residuals of the block
    pictures (delta.cut_fixture: samples of -R, 0 and R that lost planes, so that every clamp acts and the chain goes on from
    clamped samples)."""
    lo, hi = KINDS[kind][:2]
    fr = chain.frames(W, H, Cn, lo, hi, n)
    datas = chain.streams(fr)
    datas[1] = delta.cut_fixture(W, H, Cn, lo, hi, 0.6)[0]
    datas[3] = delta.cut_fixture(W, H, Cn, lo, hi, 0.33)[0]
    return fr[0], datas


_folds = {}


def oracle(datas, key, initial, W, H, Cn, lo, hi):
    k = (tuple(datas), key.tobytes(), tuple(w.tobytes() for w in initial), W, H, Cn, lo, hi)
    if k not in _folds:
        _folds[k] = chain.decode(datas, key, initial, W, H, Cn, lo, hi)
    return _folds[k]


def window_view(L, tbuf, i):
    """window i of layout L as a view [1,H,W,C] of its own"""
    lead = L.shape[:-3]
    off = L.off + (i * L.strides[0] if len(lead) == 1 else (i // lead[1]) * L.strides[0] + (i % lead[1]) * L.strides[1])
    return tbuf.as_strided((1,) + L.shape[-3:], (L.strides[-4],) + L.strides[-3:], off)


def info_fields(I):
    return (I.status, I.W, I.H, I.C, I.levels, list(I.planes), I.pmax, I.level, I.nsegs, I.truncated, list(I.missing), I.bits_used)


class Run:
    """One chain decode's buffers: the destination (prefilled) and the key, on the host and on the device."""

    def __init__(self, c, kind, Ld, Lk, key, order="rgb", seed=0):
        lo, hi, dt, sgn = KINDS[kind] if isinstance(kind, str) else kind
        self.c, self.kind, self.Ld, self.Lk, self.order = c, kind, Ld, Lk, order
        self.lo, self.hi, self.dt, self.sgn = lo, hi, dt, sgn
        self.buf = prefill(Ld.samples, kind, seed)
        self.kbuf = prefill(Lk.samples, kind, seed + 1)
        Lk.np_windows(self.kbuf)[0][...] = G.in_memory(key, order)
        self.initial = [G.in_memory(w, order).copy() for w in Ld.np_windows(self.buf)]   # (as pictures: R, G, B)
        self.tbuf, self.tkey = V.to_device(c, self.buf), V.to_device(c, self.kbuf)

    def keywords(self, stepped):
        return dict(maxval=self.hi, stepped=stepped, order=self.order, signed=self.sgn, minval=self.lo if self.sgn else None)

    def chain(self, streams, lens, stepped=False):
        return self.c.decode_view_chain(streams, lens, self.Ld.t_view(self.tbuf), self.Lk.t_view(self.tkey), **self.keywords(stepped))

    def loop(self, streams, lens, stepped=False):
        """what a caller writes without the chain call: n delta decodes of one stream each, the window before as the base.  The
        tiles of a grid's band lie side by side, row by row: their spans meet, which the delta call refuses though no sample is
        shared — there the caller's loop needs a copy of the window before, and so does this one."""
        infos = []
        beside = len(self.Ld.shape) == 5
        for i in range(self.Ld.n):
            base = window_view(self.Ld, self.tbuf, i - 1) if i else self.Lk.t_view(self.tkey)
            if i and beside:
                base = base.clone()
            infos += self.c.decode_view(streams[i:i + 1], lens[i:i + 1], window_view(self.Ld, self.tbuf, i), base=base, **self.keywords(stepped))
        return infos

    def got(self):
        return V.to_host(self.tbuf, self.dt == np.uint16), V.to_host(self.tkey, self.dt == np.uint16)

    def check_against_oracle(self, datas, key, infos):
        H, W, Cn = key.shape
        windows, links = oracle(datas, key, self.initial, W, H, Cn, self.lo, self.hi)
        want = self.buf.copy()
        for w, pic in zip(self.Ld.np_windows(want), windows):
            w[...] = G.in_memory(pic, self.order)
        T = orc.geometry(W, H).levels
        for i, (ref, I) in enumerate(zip(links, infos)):
            if ref is None:
                assert I.status != 0, i
            else:
                assert I.status == 0 and (I.level == T - 1) == (ref is not chain.UNTOUCHED), (i, I.status, I.level)
        got, gotk = self.got()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
        assert (gotk == self.kbuf).all(), "the key was written to"
        return links


def both_ways(c, kind, Ld, Lk, key, datas, stepped=False, order="rgb", seed=0):
    """The chain call against the oracle's fold, then the loop of delta calls on a second buffer with the same prefill against the
    chain call's buffer, bit for bit, with the same host_info.  -> the chain call's infos and the oracle's links."""
    streams, lens = G.to_streams(c, datas)
    a = Run(c, kind, Ld, Lk, key, order, seed)
    infos = a.chain(streams, lens, stepped)
    links = a.check_against_oracle(datas, key, infos)
    b = Run(c, kind, Ld, Lk, key, order, seed)
    infos_b = b.loop(streams, lens, stepped)
    (ga, ka), (gb, kb) = a.got(), b.got()
    assert (ga == gb).all() and (ka == kb).all()
    assert [info_fields(I) for I in infos] == [info_fields(I) for I in infos_b]
    return infos, links


# ---- decode: every layout ------------------------------------------------------------------------------------------------------

def case_inputs(case):
    (W, H), Cn, dest = case
    kname, kind = key_and_kind(case)
    (Ld, sd), (Lk, sk) = DESTS[dest](W, H, Cn), KEYS[kname](W, H, Cn)
    key, datas = chain_rows(W, H, Cn, kind, Ld.n)
    return kind, Ld, Lk, key, datas, sd or sk


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_chain_decode_equals_the_oracles_fold(ctx, case):
    """1: every destination layout against a dense, pitched, planar or stepped key; all three sample types, gray and RGB."""
    kind, Ld, Lk, key, datas, stp = case_inputs(case)
    streams, lens = G.to_streams(ctx, datas)
    r = Run(ctx, kind, Ld, Lk, key)
    links = r.check_against_oracle(datas, key, r.chain(streams, lens, stp))
    assert not any(x is None or x is chain.UNTOUCHED for x in links)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_chain_decode_equals_the_loop_of_delta_calls(ctx, case):
    """2: the same inputs through n decode_view(base=...) calls on a second buffer with the same prefill: bit for bit, host_info too."""
    kind, Ld, Lk, key, datas, stp = case_inputs(case)
    both_ways(ctx, kind, Ld, Lk, key, datas, stepped=stp, seed=2)


@pytest.mark.parametrize("dest,kname", [("dense", "planar"), ("planar", "step"), ("step", "dense"), ("tiles", "pitched")])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_chain_decode_of_bgr_pixels(ctx, wh, dest, kname):
    W, H = wh
    kind = KIND_NAMES[(SHAPES.index(wh) + len(dest)) % 3]
    (Ld, sd), (Lk, sk) = DESTS[dest](W, H, 3), KEYS[kname](W, H, 3)
    key, datas = chain_rows(W, H, 3, kind, Ld.n)
    both_ways(ctx, kind, Ld, Lk, key, datas, stepped=sd or sk, order="bgr", seed=3)


# ---- decode: a mixed batch under the switches --------------------------------------------------------------------------------------

def mixed_rows(W, H, Cn, kind):
    """7 links: whole, cut 0.6, damaged header (status 1), whole, cut before the finest level, cut 0.33, whole."""
    lo, hi = KINDS[kind][:2]
    fr = chain.frames(W, H, Cn, lo, hi, 7)
    datas = chain.streams(fr)
    datas[1] = delta.cut_fixture(W, H, Cn, lo, hi, 0.6)[0]
    datas[2] = b"\xff\xff" + datas[2][2:]
    datas[4] = levels.late_prefix(datas[4], W, H, Cn, orc.geometry(W, H).levels - 2)
    datas[5] = delta.cut_fixture(W, H, Cn, lo, hi, 0.33)[0]
    return fr[0], datas


SWITCHES = [None, ("decode_parts", 2), ("decode_parts", 4), ("one_stream", 1), ("no_square_tiles", 1), ("no_pixels16", 1), ("lift_rows", 4), ("lift_rows", 64)]


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: "plain" if s is None else "%s=%d" % s)
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_a_mixed_batch_under_the_switches(ctx, opts, wh, switch):
    """3: groups cross part boundaries and the per-image fallback runs; windows that stay are the next links' bases."""
    W, H = wh
    if switch:
        opts.set(*switch)
    for Cn, kind, dest, kname in ((1, KIND_NAMES[SHAPES.index(wh)], "stack", "dense"), (3, KIND_NAMES[(SHAPES.index(wh) + 1) % 3], "planar", "pitched")):
        (Ld, _), (Lk, _) = DESTS[dest](W, H, Cn), KEYS[kname](W, H, Cn)
        Ld = V.stack(W, H, Cn, 7) if dest == "stack" else Ld
        assert Ld.n == 7
        key, datas = mixed_rows(W, H, Cn, kind)
        infos, links = both_ways(ctx, kind, Ld, Lk, key, datas, seed=4)
        assert [x is None for x in links] == [False, False, True, False, False, False, False]
        assert [x is chain.UNTOUCHED for x in links] == [False, False, False, False, True, False, False]
        assert infos[2].status != 0 and infos[4].status == 0 and infos[4].level == orc.geometry(W, H).levels - 2


# ---- decode: the clamp fixture ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_the_clamp_fixture(ctx, wh, Cn, kind):
    """4: four links between two block pictures, every one cut: each meets every clamp on the running decoded base, and from link 2
    on a quarter of the samples or more would differ had the true previous frame been the base (tests/test_chain_cpu.py)."""
    W, H = wh
    lo, hi = KINDS[kind][:2]
    key, datas, _ = chain.clamp_fixture(W, H, Cn, lo, hi)
    n = len(datas) + 1   # (and a whole link after the four, on a base that is nothing but clamped samples)
    fr = chain.frames(W, H, Cn, lo, hi, 2)
    datas = datas + [delta.stream(fr[2], fr[1])[0]]
    Ld = G.dense(W, H, Cn, n) if Cn == 1 else V.stack(W, H, Cn, n)
    (Lk, _) = KEYS["pitched" if Cn == 1 else "dense"](W, H, Cn)
    both_ways(ctx, kind, Ld, Lk, key, datas, seed=5)


# ---- decode: one link ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_one_link_is_the_delta_call(ctx, wh, Cn):
    """5: n == 1 against decode_view(base=key), bit for bit — dense pairs (the fused sinks where the shape has them) and a pitched one."""
    W, H = wh
    for kind, Ld, kname in ((KIND_NAMES[SHAPES.index(wh)], G.dense(W, H, Cn, 1), "dense"), (KIND_NAMES[(SHAPES.index(wh) + 1) % 3], V.stack(W, H, Cn, 1), "pitched")):
        Lk = KEYS[kname](W, H, Cn)[0]
        lo, hi = KINDS[kind][:2]
        for data in (chain_rows(W, H, Cn, kind, 4)[1][0], delta.cut_fixture(W, H, Cn, lo, hi, 0.6)[0]):
            key = chain.frames(W, H, Cn, lo, hi, 4)[0]
            both_ways(ctx, kind, Ld, Lk, key, [data], seed=6)


# ---- round trips of one stack -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KIND_NAMES)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_round_trip_of_a_stack_with_its_first_frame_as_key(ctx, wh, Cn, kind):
    """6: `t[0]` as key and `t[1:]` as destination of ONE stack: encode_view_chain, then decode_view_chain into a copy whose frames
    1.. are random samples."""
    import torch

    W, H = wh
    n = 6
    lo, hi, dt, sgn = KINDS[kind]
    fr = chain.frames(W, H, Cn, lo, hi, n)
    t = V.to_device(ctx, np.stack(fr))
    out, info = ctx.encode_view_chain(t[1:], t[0], signed=sgn)
    assert all(I.error == 0 for I in V.infos_of(info))
    back = V.to_device(ctx, prefill(t.numel(), kind, 7).reshape(t.shape))
    back[0] = t[0]
    infos = ctx.decode_view_chain(out, ctx.stream_lengths(info), back[1:], back[0], maxval=hi, signed=sgn, minval=lo if sgn else None)
    assert [I.status for I in infos] == [0] * n
    assert torch.equal(back, t) and (V.to_host(t, dt == np.uint16) == np.stack(fr)).all()


@pytest.mark.parametrize("sgn", [0, 1], ids=["uint16", "int16"])
def test_round_trip_of_a_full_range_stack(ctx, sgn):
    """6: frames over the whole range of the type, whose residuals leave int16."""
    import torch

    W, H, n = 132, 72, 5
    kind = (-32768, 32767, np.int16, True) if sgn else (0, 65535, np.uint16, False)
    fr = chain.full_range_frames(W, H, sgn, n)
    t = V.to_device(ctx, np.stack(fr))
    out, info = ctx.encode_view_chain(t[1:], t[0], signed=bool(sgn))
    G.check_streams(out, info, [(fr[i + 1], fr[i]) for i in range(n)], prefilled=False)
    back = V.to_device(ctx, prefill(t.numel(), kind, 8).reshape(t.shape))
    back[0] = t[0]
    infos = ctx.decode_view_chain(out, ctx.stream_lengths(info), back[1:], back[0], maxval=kind[1], signed=bool(sgn), minval=kind[0] if sgn else None)
    assert [I.status for I in infos] == [0] * n and torch.equal(back, t)


# ---- encode ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in CASES if c[2] in ("dense", "tiles", "planar", "step")], ids=_case_id)
def test_chain_encode_equals_the_oracle_and_the_two_delta_calls(ctx, case):
    """7: streams and records equal the oracle's residual streams and the two delta encodes byte for byte, whole buffers, with and
    without a capacity of 500."""
    import torch

    (W, H), Cn, dest = case
    kname, kind = key_and_kind(case)
    lo, hi, dt, sgn = KINDS[kind]
    (Ls, sd), (Lk, sk) = DESTS[dest](W, H, Cn), KEYS[kname](W, H, Cn)
    stp, n = sd or sk, Ls.n
    fr = chain.frames(W, H, Cn, lo, hi, n)
    fr = fr[:2] + [delta.clamp_pair(W, H, Cn, lo, hi)[0]] + fr[3:]   # (one block picture: residuals of the whole range around it)
    bufS, tS = G.load(ctx, Ls, fr[1:], dt)
    bufK, tK = G.load(ctx, Lk, fr[:1], dt, salt=1)
    src, key = Ls.t_view(tS), Lk.t_view(tK)
    stride = ctx.lib.dwtx_encode_bound16(W, H, Cn)
    for capacity in (0, 500):
        shape = (n, stride if capacity <= 0 else (capacity + 15) // 8 * 8)
        out = torch.full(shape, G.FILL, dtype=torch.uint8, device=ctx.device)
        out, info = ctx.encode_view_chain(src, key, capacity, out=out, stepped=stp, signed=sgn)
        G.check_streams(out, info, [(fr[i + 1], fr[i]) for i in range(n)], capacity)
        two, two_info = torch.full(shape, G.FILL, dtype=torch.uint8, device=ctx.device), torch.zeros_like(info)
        ctx.encode_view(window_view(Ls, tS, 0), capacity, out=two[:1], info=two_info[:1], stepped=stp, signed=sgn, base=key)
        rest = torch.full((n - 1, shape[1]), G.FILL, dtype=torch.uint8, device=ctx.device)
        rest_info = torch.zeros_like(info[1:])
        for i in range(1, n):   # (window by window: a tile grid's windows 1.. are no grid of their own)
            ctx.encode_view(window_view(Ls, tS, i), capacity, out=rest[i - 1:i], info=rest_info[i - 1:i], stepped=stp, signed=sgn, base=window_view(Ls, tS, i - 1))
        assert torch.equal(out[:1], two[:1]) and torch.equal(out[1:], rest)
        assert [V.fields(I) for I in V.infos_of(info)] == [V.fields(I) for I in V.infos_of(two_info[:1]) + V.infos_of(rest_info)]
    assert (V.to_host(tS, dt == np.uint16) == bufS).all() and (V.to_host(tK, dt == np.uint16) == bufK).all(), "a source was written to"


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_chain_encode_of_a_stack_equals_two_delta_calls(ctx, Cn):
    """7: on a stack the second delta call is `t[2:]` against `t[1:-1]` in one piece."""
    import torch

    W, H, n, kind = 132, 72, 6, "u8"
    lo, hi, dt, sgn = KINDS[kind]
    fr = chain.frames(W, H, Cn, lo, hi, n)
    t = V.to_device(ctx, np.stack(fr))
    out, info = ctx.encode_view_chain(t[1:], t[0])
    a, ia = ctx.encode_view(t[1:2], base=t[0:1])
    b, ib = ctx.encode_view(t[2:], base=t[1:-1])
    lens = ctx.stream_lengths(info)
    assert torch.equal(lens, torch.cat([ctx.stream_lengths(ia), ctx.stream_lengths(ib)]))
    two = torch.cat([a, b])
    for i in range(n):
        k = int(lens[i])
        assert torch.equal(out[i, :k], two[i, :k]), i
    assert [V.fields(I) for I in V.infos_of(info)] == [V.fields(I) for I in V.infos_of(torch.cat([ia, ib]))]


@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_the_encode_index_lands_at_entry_i_and_the_decode_takes_it(ctx, opts, Cn):
    """7: the index of stream i at entry i across the two encodes of the composition; the chain decode is offered them with
    no_index_fallback set (an index that is turned down is then an error)."""
    import torch

    import dwt_amd

    W, H, n, kind = 132, 72, 5, "u8"
    lo, hi, dt, sgn = KINDS[kind]
    fr = chain.frames(W, H, Cn, lo, hi, n)
    t = V.to_device(ctx, np.stack(fr))
    dev_index = ctx.set_encode_index(n, device=True)
    try:
        out, info = ctx.encode_view_chain(t[1:], t[0])
        enc = [dwt_amd.index_from_row(dev_index[i]) for i in range(n)]
    finally:
        ctx.set_encode_index()
    assert all(X.magic == dwt_amd.INDEX_MAGIC and X.nsegs > 0 and (X.W, X.H, X.C) == (W, H, Cn) for X in enc)
    lens = ctx.stream_lengths(info)
    alone = []
    for i in range(n):   # each stream's own index, from a delta encode of it alone
        one = ctx.set_encode_index(1, device=True)
        try:
            ctx.encode_view(t[i + 1:i + 2], base=t[i:i + 1])
            alone.append(dwt_amd.index_from_row(one[0]))
        finally:
            ctx.set_encode_index()
    def index_fields(X):   # (an encode writes an entry's header and seg[:nsegs], nothing behind them)
        return (X.magic, X.W, X.H, X.C, X.nsegs, X.stream_bits, [(s.bit, s.sym_base, s.n1, s.cnt, s.desc, s.order) for s in X.seg[:X.nsegs]])

    assert len({X.stream_bits for X in enc}) == n   # (five streams of five lengths: an entry in the wrong place shows)
    assert [index_fields(X) for X in enc] == [index_fields(X) for X in alone]
    back = V.to_device(ctx, prefill(t.numel(), kind, 9).reshape(t.shape))
    back[0] = t[0]
    opts.set("no_index_fallback", 1)
    ctx.set_index((dwt_amd.Index * n)(*enc), 0)
    try:
        infos = ctx.decode_view_chain(out, lens, back[1:], back[0])
    finally:
        ctx.set_index()
    assert [I.status for I in infos] == [0] * n and torch.equal(back, t)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_with_their_texts_and_nothing_written(ctx):
    """8"""
    import torch

    import dwt_amd

    W, H, n = 132, 72, 3
    t = torch.full((n + 1, H, W, 1), 7, dtype=torch.uint8, device=ctx.device)
    other = torch.full((1, H, W, 1), 9, dtype=torch.uint8, device=ctx.device)
    streams = torch.zeros((n, 4096), dtype=torch.uint8, device=ctx.device)
    lens = torch.full((n,), 100, dtype=torch.int64, device=ctx.device)
    out = torch.full((n, 4096), 3, dtype=torch.uint8, device=ctx.device)

    def refused(text, fn):
        with pytest.raises(dwt_amd.DwtxError) as e:
            fn()
        assert e.value.rc == ERR_ARG and text in str(e.value), str(e.value)

    # the key meets the destination: it is a window of it, or lies one row down into one
    refused("window 0 of the destination meets the key", lambda: ctx.decode_view_chain(streams, lens, t[:-1], t[0]))
    refused("window 2 of the destination meets the key", lambda: ctx.decode_view_chain(streams, lens, t[:-1], t[2]))
    shifted = t.reshape(-1).as_strided((1, H, W, 1), (H * W, W, 1, 1), H * W + W)
    refused("window 1 of the destination meets the key", lambda: ctx.decode_view_chain(streams, lens, t[:-1], shifted))
    # a NULL key, mismatched channels and sample sizes: the C calls say so themselves
    lib, Cc = ctx.lib, dwt_amd.C
    v, vW, vH, Cn, vn, step = ctx._view(t[1:], 255)
    infos = (dwt_amd.DecodeInfo * n)()
    info = torch.zeros((n, Cc.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)

    def c_decode(key):
        return lib.dwtx_decode_view_chain(ctx.h, streams.data_ptr(), streams.shape[1], lens.data_ptr(), W, H, n, Cc.byref(v), step, key, 0, 0, 0, 0,
                                          Cc.cast(infos, Cc.c_void_p))

    def c_encode(key):
        return lib.dwtx_encode_view_chain(ctx.h, Cc.byref(v), step, key, 0, 0, 0, W, H, n, 0, out.data_ptr(), out.shape[1], info.data_ptr())

    def key_view(**changes):
        f = dict(dev=other.data_ptr(), sample_bytes=1, channels=1, maxval=255, cols=0, row_pitch=W, image_stride=0, band_stride=0, channel_stride=0)
        f.update(changes)
        return dwt_amd.View(f["dev"], f["sample_bytes"], f["channels"], f["maxval"], f["cols"], f["row_pitch"], f["image_stride"], f["band_stride"],
                            f["channel_stride"])

    for call in (c_decode, c_encode):
        for key, text in ((None, "no key"), (Cc.byref(key_view(dev=None)), "no key"), (Cc.byref(key_view(channels=3, row_pitch=3 * W)), "1 channels, its key 3"),
                          (Cc.byref(key_view(sample_bytes=2)), "1-byte samples, its key 2-byte")):
            assert call(key) == ERR_ARG and text in lib.dwtx_last_error().decode(), lib.dwtx_last_error()
    # sgn with bytes; 8-bit samples have one maxval; a signed range must be one
    assert lib.dwtx_decode_view_chain(ctx.h, streams.data_ptr(), streams.shape[1], lens.data_ptr(), W, H, n, Cc.byref(v), step, Cc.byref(key_view()), 0, 0, 1, 0,
                                      Cc.cast(infos, Cc.c_void_p)) == ERR_ARG and "int16_t" in lib.dwtx_last_error().decode()
    refused("maxval 100", lambda: ctx.decode_view_chain(streams, lens, t[1:], other, maxval=100))
    s16 = torch.zeros((n, H, W, 1), dtype=torch.int16, device=ctx.device)
    refused("minval < maxval", lambda: ctx.decode_view_chain(streams, lens, s16, torch.zeros_like(s16[:1]), signed=True, minval=50, maxval=10))
    assert (t == 7).all() and (other == 9).all() and not s16.any() and (out == 3).all() and not info.any()
    # in Python, before any device call: the keywords of the other view calls, lists, floats, a missing key, another dtype or shape
    bad = [dict(key=other, flip="y"), dict(key=other, levels_max=2), dict(key=other, crop=(64, 64)), dict(key=other, base=t[:-1]),
           dict(key=None), dict(key=other.to(torch.int16)), dict(key=other[:, :, :64]), dict(key=other.float()), dict(key=t[:2])]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.decode_view_chain(streams, lens, t[1:], **kw)
        if "levels_max" not in kw and "crop" not in kw:
            with pytest.raises(ValueError):
                ctx.encode_view_chain(t[1:], **kw)
    for into in (t[1:].float(), [t[1], t[2], t[3]]):
        with pytest.raises(ValueError):
            ctx.decode_view_chain(streams, lens, into, other.float() if hasattr(into, "dtype") else other)
    assert (t == 7).all() and (other == 9).all()


# ---- the context's history ---------------------------------------------------------------------------------------------------------

@pytest.fixture
def fresh(ctx):
    """A context that has run nothing yet (it depends on `ctx`: no GPU, no test)"""
    import dwt_amd

    c = dwt_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("Cn,kind", [(1, "s16"), (3, "u8")], ids=["gray-s16", "rgb-u8"])
def test_a_chain_call_after_calls_of_another_geometry_channel_count_and_depth(fresh, Cn, kind):
    """9: tests/history.py's dirt — noise of more planes, at least as large in every dimension a slot is sized by — of the other
    channel count, a transposed geometry and 16-bit depth on a private context, then the chain call, whole result compared."""
    W, H = 263, 135
    n = 7
    key, datas = mixed_rows(W, H, Cn, kind)
    stride = history.stride_of(datas)
    for cl in (history.call("decode", W, H, 3, n=8, stride=stride), history.call("decode16", H + 1, W + 1, 4 - Cn, n=8, stride=stride),
               history.call("decode", W, H, Cn, n=8, stride=stride), history.call("encode", W, H, Cn, n=8)):
        history.dirty(fresh, cl.W, cl.H, cl.Cn, cl.n, cl.how, cl.kind, cl.stride)
    Ld, Lk = V.stack(W, H, Cn, n), KEYS["pitched"](W, H, Cn)[0]
    both_ways(fresh, kind, Ld, Lk, key, datas, seed=10)


@pytest.mark.parametrize("Cn,kind", [(1, "u16"), (3, "s16")], ids=["gray-u16", "rgb-s16"])
def test_a_chain_call_as_a_contexts_first_call(fresh, Cn, kind):
    """9"""
    W, H = 263, 135
    key, datas = mixed_rows(W, H, Cn, kind)
    streams, lens = G.to_streams(fresh, datas)
    r = Run(fresh, kind, V.stack(W, H, Cn, 7), KEYS["dense"](W, H, Cn)[0], key, seed=11)
    r.check_against_oracle(datas, key, r.chain(streams, lens))
