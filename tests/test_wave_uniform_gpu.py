"""GPU: kernels that give one wave one item take the wave's index inside the workgroup as a scalar (wave_in_block(),
dwtx_internal.h), and k_code / k_apply_all take a plane's facts from lane registers as scalars.  What could go wrong: an
index assumed the same for a wave is not, or a wave takes its neighbour's item — which shows where the waves of one
workgroup do different things.  So the shapes here put, into the same workgroups,
  - idle waves beside working ones: tile counts NT with NT % 4 = 1, 2, 3 (and 0: 1024x1024, all whole squares),
  - tiles that are whole 32x32 squares of the pyramid beside tiles the ring's edges cut (1056 = 1024 + 32 has curve
    squares of side 2048: squares inside, cut blocks along the border),
  - levels with fewer tiles than a workgroup has waves (every shape's coarse levels are one tile each),
  - three channels.
NT is computed here from the geometry and the set is asserted to cover the four remainders.  Every comparison is exact and
against the oracle: streams, pixels, coefficient planes and pyramids."""
import functools

import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu

# W, H, C; NT % 4 = 1, 1, 0, 0, 2, 2, 2, 2 and, with 136x104 (27 tiles), 3
SHAPES = [(72, 40, 1), (104, 104, 3), (288, 544, 1), (544, 288, 3), (1056, 1056, 1), (1056, 1056, 3), (2080, 1056, 1), (1024, 1024, 1),
          (136, 104, 3)]
N = 5   # frames of a batch: the decoder cuts batches of 4 to 23 into two parts


def tiles_per_level(W, H):
    """dwtx_tiles restated: the non-empty 32x32 curve blocks of every ring level -> [(tiles, whole squares among them)].
    A block of the level's lengths[l+1]-sided curve square holds ring coefficients if it reaches into the level's
    widths[l+1] x heights[l+1] rectangle and does not lie wholly inside the LL quadrant; levels up to 32x32 are one block."""
    g = orc.geometry(W, H)
    out = []
    for l in range(g.levels):
        n, w0, h0, w1, h1 = g.lengths[l + 1], g.widths[l], g.heights[l], g.widths[l + 1], g.heights[l + 1]
        if n <= 32:
            out.append((1, 0))
            continue
        bx, by = np.meshgrid(np.arange(n // 32) * 32, np.arange(n // 32) * 32)
        inside = (bx < w1) & (by < h1) & ~((bx + 32 <= w0) & (by + 32 <= h0))
        whole = (bx + 32 <= w1) & (by + 32 <= h1) & ((bx >= w0) | (by >= h0))
        out.append((int(inside.sum()), int(whole.sum())))
    return out


def test_the_shapes_create_the_conditions():
    rem, mixed = set(), 0
    for W, H, Cn in SHAPES:
        per = tiles_per_level(W, H)
        NT = sum(t for t, _ in per)
        print(f"{W}x{H}x{Cn}: NT = {NT} (NT % 4 = {NT % 4}), tiles / whole squares per level {per}")
        rem.add(NT % 4)
        assert sum(1 for t, _ in per if t < 4) >= 2, "levels with fewer tiles than a workgroup has waves"
        mixed += any(0 < sq < t for t, sq in per) and W % 4 == 0
    assert rem == {0, 1, 2, 3}
    assert mixed >= 4, "workgroups with whole-square tiles and border-cut tiles together"
    assert tiles_per_level(1024, 1024)[-1] == (768, 768) and {Cn for _, _, Cn in SHAPES} == {1, 3}


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
    """k_code<false>, k_apply_all and every wave-per-item kernel around them: encode_device of five frames gives the oracle's
    bytes, decode_device (two decoder parts) the pixels back with status 0, decode_planes the oracle's coefficients."""
    assert len(deep.decoder_parts(N)) == 2
    _codec_8bit(ctx, *shape)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_codec_8bit_linearised_tiles(ctx, shape, opts):
    """The same with DWTX_OPT_NO_SQUARE_TILES: every tile of the same kernels through the linearised copy."""
    opts.set("no_square_tiles", 1)
    _codec_8bit(ctx, *shape)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_codec_16bit(ctx, shape):
    """Deep pixels reach k_code<true>, whose waves loop over several tiles: encode_device16 gives the composed oracle's bytes,
    decode_device16 the pixels back, decode_planes the oracle's coefficients (more than eight planes per channel)."""
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


def _planes(a):
    """interleaved [H, W, C] -> planar [C, H, W]"""
    return np.ascontiguousarray(a.transpose(2, 0, 1))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_transforms(ctx, shape):
    """The lifting kernels (wide levels, narrow levels, tails) on the same shapes: transformation_fwd / _inv of int32 planes
    and transformation_fwd_pixels / _inv_pixels of 8-bit pixels against orc.forward / orc.inverse."""
    import torch

    W, H, Cn = shape
    n = 2
    g = orc.geometry(W, H)
    rng = np.random.default_rng(W * 3 + H + Cn)
    a = rng.integers(-300, 300, size=(n, H, W, Cn), dtype=np.int32)
    fwd = np.concatenate([_planes(orc.forward(x)) for x in a])
    inv = np.concatenate([_planes(orc.inverse(x)) for x in a])
    t = torch.from_numpy(np.concatenate([_planes(x) for x in a])).to(ctx.device)
    assert (ctx.transformation_fwd(t).cpu().numpy() == fwd).all()
    assert (ctx.transformation_inv(t).cpu().numpy() == inv).all()
    pix = _pictures(W, H, Cn)[:n]
    p = torch.from_numpy(np.array(pix)).to(ctx.device)
    for rings16 in (True, False):
        pyr, r16, mask = ctx.transformation_fwd_pixels(p, rings16=rings16)
        got = pyr.cpu().numpy()
        if mask:
            r = r16.cpu().numpy()
            for l in range(g.levels):
                if (mask >> l) & 1:
                    w0, h0, w1, h1 = g.widths[l], g.heights[l], g.widths[l + 1], g.heights[l + 1]
                    got[:, :h1, w0:w1] = r[:, :h1, w0:w1]
                    got[:, h0:h1, :w0] = r[:, h0:h1, :w0]
        want = np.concatenate([_planes(orc.stage_dump(x)[0]) for x in pix])
        assert (got == want).all(), rings16
        assert torch.equal(ctx.transformation_inv_pixels(pyr, r16, mask, Cn), p), rings16
