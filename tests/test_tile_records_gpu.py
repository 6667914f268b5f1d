"""GPU: the entropy stage's kernels take a tile's level, ring offset, coefficient count and square map from one 16-byte
record of the plan (dwtx_tile_rec, dwtx_internal.h) instead of working them out per wave.  A wrong record shows as wrong
coefficients, so every check is exact and against the oracle: encode_device streams equal orc.encode, decode_device pixels
equal the source, decode_planes coefficients equal orc.decode_stage.  The shapes are the smallest that reach each thing a
record holds:
  - levels of side <= 32 only (the empty map, one tile per level): 24x24, 32x32;
  - curve squares of side 64, 128, 256 (one to three iterations of the map's recursion, all four quadrant cases and both
    swap states among the whole squares): 64x64, 128x128, 256x256, and 200x136 with cut blocks (cnt < 1024) beside them;
  - whole squares beside border-cut tiles at side 2048: 1056x1056, and 2080x1056 (side 4096, not square);
  - deep maps with few tiles: 8256x72 (side 16384, nine iterations) and 16456x72 (side 32768, ten iterations, the top bit
    of the record's 16-bit masks in use), both with whole squares in the finest ring;
  - a width that is no multiple of 4 (no square path: base, cnt and level alone carry the tile): 1001x37.
The geometry is restated here from orc.geometry and the set is asserted to produce these conditions.  (The seven-iteration
map of a 4096x4096 frame is the golden tests'.)"""
import functools

import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu

SMALL = [(24, 24, 1), (24, 24, 3), (32, 32, 1), (32, 32, 3)]
CURVE = [(64, 64, 1), (128, 128, 1), (256, 256, 1), (200, 136, 1)]
BORDER = [(1056, 1056, 1), (1056, 1056, 3), (2080, 1056, 1)]
DEEP_MAPS = [(8256, 72, 1), (16456, 72, 1)]
NO_SQUARES = [(1001, 37, 3)]
SHAPES = SMALL + CURVE + BORDER + DEEP_MAPS + NO_SQUARES
N = 5   # frames of a batch: the decoder cuts batches of 4 to 23 into two parts


def square_maps(n, d):
    """hilbert_dev.h square_map restated for an array of curve blocks d of a level with outer side n ->
    (swap, mx, my, iterations, the quadrant case rx * 2 + ry of every block at every iteration)"""
    d = d.astype(np.uint32)
    sw, mx, my = np.zeros(d.shape, bool), np.zeros(d.shape, np.uint32), np.zeros(d.shape, np.uint32)
    cases, s = [], 32
    while s < n:
        rx = (d >> 1) & 1
        ry = (d ^ rx) & 1
        flip = (rx == 1) & (ry == 0)
        mx, my = np.where(flip, mx ^ np.uint32(s - 1), mx), np.where(flip, my ^ np.uint32(s - 1), my)
        swap = ry == 0
        mx, my = np.where(swap, my, mx), np.where(swap, mx, my)
        sw = sw ^ swap
        mx, my = mx ^ (rx * s).astype(np.uint32), my ^ (ry * s).astype(np.uint32)
        cases.append(rx * 2 + ry)
        d = d >> 2
        s <<= 1
    return sw, mx, my, len(cases), cases


def level_facts(W, H):
    """Per ring level: outer side, iterations of the map, tiles, whole squares among them, and over the whole squares the swap
    states, the quadrant cases and the largest XOR mask.  A block holds ring coefficients if it reaches into the level's
    widths[l+1] x heights[l+1] rectangle and does not lie wholly inside the LL quadrant; levels up to 32x32 are one tile."""
    g = orc.geometry(W, H)
    out = []
    for l in range(g.levels):
        n, w0, h0, w1, h1 = g.lengths[l + 1], g.widths[l], g.heights[l], g.widths[l + 1], g.heights[l + 1]
        if n <= 32:
            out.append(dict(side=n, iters=0, tiles=1, whole=0, swaps=set(), cases=set(), mask=0))
            continue
        sw, mx, my, iters, cases = square_maps(n, np.arange((n // 32) ** 2))
        bx, by = (mx & ~np.uint32(31)).astype(np.int64), (my & ~np.uint32(31)).astype(np.int64)
        inside = (bx < w1) & (by < h1) & ~((bx + 32 <= w0) & (by + 32 <= h0))
        whole = (bx + 32 <= w1) & (by + 32 <= h1) & ((bx >= w0) | (by >= h0))
        seen = set()
        for c in cases:
            seen |= set(np.unique(c[whole]).tolist())
        mask = int(max(mx[whole].max(initial=0), my[whole].max(initial=0)))
        out.append(dict(side=n, iters=iters, tiles=int(inside.sum()), whole=int(whole.sum()), swaps=set(sw[whole].tolist()), cases=seen, mask=mask))
    return out


def test_the_shapes_create_the_conditions():
    facts = {}
    for W, H, Cn in SHAPES:
        facts[W, H] = f = level_facts(W, H)
        print(f"{W}x{H}x{Cn}: " + "; ".join(f"side {x['side']}: {x['tiles']} tiles, {x['whole']} whole, {x['iters']} iterations, mask {x['mask']:#x}" for x in f))
    for W, H, _ in SMALL:
        assert all(x["side"] <= 32 and x["tiles"] == 1 for x in facts[W, H])
    assert {Cn for _, _, Cn in SMALL} == {1, 3}
    # one, two and three iterations; the four quadrant cases and both swap states among whole squares
    for (W, H, _), side in zip(CURVE[:3], (64, 128, 256)):
        fine = facts[W, H][-1]
        assert fine["side"] == side and fine["iters"] == {64: 1, 128: 2, 256: 3}[side] and fine["whole"] == fine["tiles"] > 0
        assert fine["swaps"] == {False, True}
    assert facts[64, 64][-1]["cases"] == {1, 2, 3} and facts[128, 128][-1]["cases"] == {0, 1, 2, 3} and facts[256, 256][-1]["cases"] == {0, 1, 2, 3}
    cut = facts[200, 136][-1]
    assert cut["side"] == 256 and 0 < cut["whole"] < cut["tiles"] and cut["swaps"] == {False, True} and cut["cases"] == {0, 1, 2, 3}
    # whole squares beside border-cut tiles at side 2048 (and 4096 for the frame that is not square)
    assert facts[1056, 1056][-1]["side"] == 2048 and facts[2080, 1056][-2]["side"] == 2048 and facts[2080, 1056][-1]["side"] == 4096
    for W, H, _ in BORDER:
        assert all(0 < x["whole"] < x["tiles"] for x in facts[W, H] if x["side"] >= 1024)
    assert {Cn for W, _, Cn in BORDER if W == 1056} == {1, 3}
    # deep maps with few tiles: nine and ten iterations, whole squares in the finest ring, bit 14 of a mask set
    for (W, H, _), side, iters in zip(DEEP_MAPS, (16384, 32768), (9, 10)):
        fine = facts[W, H][-1]
        assert fine["side"] == side and fine["iters"] == iters and fine["whole"] > 0 and fine["tiles"] < 1500
        assert fine["swaps"] == {False, True} and fine["cases"] == {0, 1, 2, 3}
        assert fine["mask"] >> (iters + 4) == 1, "the top bit the level's masks can have is in use"
        assert W % 4 == 0 and W * H <= 1200000
    assert facts[16456, 72][-1]["mask"] >> 14 == 1 and facts[16456, 72][-1]["mask"] < 1 << 15
    # no square path, yet tiles of 1024 coefficients beside shorter ones and three channels
    (W, H, Cn), = NO_SQUARES
    assert W % 4 != 0 and Cn == 3 and any(x["tiles"] > 4 for x in facts[W, H])


@functools.lru_cache(maxsize=None)
def _pictures(W, H, Cn):
    pix = np.stack([orc.synth(W, H, Cn, 3 + i, 0) for i in range(N)])
    pix.setflags(write=False)
    return pix


@functools.lru_cache(maxsize=None)
def _oracle(W, H, Cn):
    """(streams, decode_stage of every stream): computed once per shape, shared by the tests below"""
    streams = [orc.encode(p)[0] for p in _pictures(W, H, Cn)]
    return streams, [orc.decode_stage(s, W, H, Cn) for s in streams]


def _codec_8bit(ctx, W, H, Cn):
    import torch

    pix = _pictures(W, H, Cn)
    want, stages = _oracle(W, H, Cn)
    t = torch.from_numpy(np.array(pix)).to(ctx.device)
    out, info = ctx.encode_device(t)
    lens = ctx.stream_lengths(info)
    host, hl = out.cpu().numpy(), lens.cpu().numpy()
    for i in range(N):
        assert host[i, :hl[i]].tobytes() == want[i], i
    back, infos = ctx.decode_device(out, lens, W, H, Cn)
    assert [I.status for I in infos] == [0] * N
    assert torch.equal(back.view(N, H, W, Cn), t)
    lin, infos = ctx.decode_planes(want, W, H, Cn)
    lin = lin.cpu().numpy().reshape(N, Cn, W * H)
    for i, (rlin, level, missing, planes) in enumerate(stages):
        assert infos[i].status == 0 and infos[i].level == level and list(infos[i].planes)[:Cn] == planes, i
        assert list(infos[i].missing) == missing.tolist(), i
        assert (lin[i] == rlin).all(), i


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_codec_8bit(ctx, shape):
    """k_hist, k_code<false>, k_count, k_apply_all and the per-lane readers of the records: encode_device of five frames gives
    the oracle's bytes, decode_device (two decoder parts) the pixels back with status 0, decode_planes the oracle's coefficients."""
    assert len(deep.decoder_parts(N)) == 2
    _codec_8bit(ctx, *shape)


@pytest.mark.parametrize("shape", CURVE + BORDER[:1] + DEEP_MAPS + NO_SQUARES, ids=lambda s: "%dx%dx%d" % s)
def test_codec_8bit_linearised_tiles(ctx, shape, opts):
    """The same with DWTX_OPT_NO_SQUARE_TILES: every tile through the linearised copy, at the record's ring offset."""
    opts.set("no_square_tiles", 1)
    _codec_8bit(ctx, *shape)


@pytest.mark.parametrize("shape", [(256, 256, 1), (200, 136, 1), (16456, 72, 1), (1001, 37, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_codec_16bit(ctx, shape):
    """Deep pixels reach k_code<true>, whose waves loop over several tiles with a record each: encode_device16 gives the
    composed oracle's bytes, decode_device16 the pixels back, decode_planes the oracle's coefficients."""
    import torch

    W, H, Cn = shape
    M = 65535
    pics = [deep.smooth_noise(W, H, Cn, 16383, 1), deep.blocks(W, H, Cn, 4095, 2), deep.noise(W, H, Cn, 1023, 3), deep.smooth_noise(W, H, Cn, M, 4),
            deep.blocks(W, H, Cn, 4095, 5)]
    want = [deep.deep_encode(p) for p in pics]
    assert all(8 < k <= 16 for _, st in want for k in list(st.planes)[:Cn])   # every plane is the wide kernel's
    t = torch.from_numpy(np.stack(pics)).to(ctx.device)
    out, info = ctx.encode_device16(t)
    lens = ctx.stream_lengths(info)
    host, hl = out.cpu().numpy(), lens.cpu().numpy()
    for i in range(N):
        assert host[i, :hl[i]].tobytes() == want[i][0], i
    back, infos = ctx.decode_device16(out, lens, W, H, Cn, M)
    assert [I.status for I in infos] == [0] * N
    assert (back.cpu().numpy().reshape(N, H, W, Cn) == np.stack(pics)).all()
    lin, infos = ctx.decode_planes([w for w, _ in want], W, H, Cn)
    lin = lin.cpu().numpy().reshape(N, Cn, W * H)
    for i, (w, _) in enumerate(want):
        rlin, level, missing, planes = orc.decode_stage(w, W, H, Cn)
        assert infos[i].status == 0 and infos[i].level == level and list(infos[i].planes)[:Cn] == planes, i
        assert (lin[i] == rlin).all(), i
