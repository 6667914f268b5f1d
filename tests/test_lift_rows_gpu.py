"""GPU: the lifting kernels at every rows-per-wave setting, at the edges of their row logic.

Every lifting launch of lift.hip takes its row pairs per wave strip from the size of the BATCH (fill_chip / pick_rpw:
64 halved down to 4 while fewer than 4096 waves would run; the two-level kernels 8 down to 2), so a test with a few
small planes only ever runs the floor values, whatever its shape.  DWTX_OPT_LIFT_ROWS ("lift_rows") forces the value a
large batch gets: R = 8 / 16 / 32 / 64 row pairs for the one-level kernels, M = max(2, R / 8) coarse row pairs for the
two-level ones.  What depends on it (lift.hip): a strip's halo pair (jfirst = j0 - 1), where the batches of S = 2 row
pairs end against j1 = min(j0 + R, h2), which wave gets the pair whose odd row does not exist, how many row pairs lie
between two histogram flushes, which waves of a block leave at once (j0 >= h2).

Every comparison is exact and against the CPU oracle (orc.*; tests/deep.py's pair for 16-bit samples); that the forced
run gives the bytes of the automatic one is checked on top of that, never instead."""
import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu

ROWS = (8, 16, 32, 64)   # 4 is what every other small-batch test runs
M16 = 4095


def mpw_of(R):
    return max(2, R // 8)


# ---- a. int32 planes ---------------------------------------------------------------------------------------------

# The one-level kernels (k_fwd_level_w / k_inv_level_w, and k_fwd_level / k_inv_level where W % 4 != 0): wave strip s of
# a column of strips makes the row pairs s*R .. min(s*R + R, h2) - 1 of the h2 = ceil(H / 2) the level has, WAVES = 4
# strips to a block where the waves are stacked (always in the inverse; in the forward wide kernel 4 >> wx_log2).
# Coarse heights of the finest level, for a forced R:
EDGES = (
    ("R-1", lambda R: R - 1),        # one strip, cut short; three waves of the block leave at once
    ("R", lambda R: R),              # one strip, exact: its last batch of two pairs is whole
    ("R+1", lambda R: R + 1),        # a second strip of ONE pair, whose halo pair is the first strip's last
    ("2R+1", lambda R: 2 * R + 1),   # a third strip (the second block where wx_log2 = 1 stacks two waves)
    ("4R-1", lambda R: 4 * R - 1),   # a whole block of four strips, the last one cut short
    ("4R+1", lambda R: 4 * R + 1),   # ... followed by a second block of one strip of one pair
)
# each with H = 2 h2 (every pair whole) and H = 2 h2 - 1 (the last pair has no odd row: its strip must not read or write it).
# The coarser levels of the same picture run the same R at whatever heights halving gives them.
# Widths of the wide kernels: 8 = one quad, 12 = three quads (both wx_log2 = 0: four waves stacked), 260 = 65 quads, one
# lane into a second 64-quad strip (wx_log2 = 1: two by two), 772 = 193 quads, four strips side by side (wx_log2 = 2; the
# inverse, 64 quads per wave and no wx, takes four blocks in x).  Their coarser levels (130, 65; 386, 193; 6, 3) are narrow.
WIDE_W = (8, 260, 12, 772)
# Widths of the narrow kernels (W % 4 != 0; 64 column pairs per forward wave, INV_PAIRS = 62 per inverse wave): 9 = five
# pairs, the last without an odd column; 126 = 63 pairs, one past INV_PAIRS and one short of the forward wave; 131 = 66 pairs,
# two past the forward wave, odd.
NARROW_W = (9, 126, 131)


def one_level_cases():
    """(R, W, H): every R meets every edge, even and odd, in two wide widths and one narrow one; the widths rotate so
    that each of them meets every edge under some R and every R at some edge."""
    cases = []
    for r, R in enumerate(ROWS):
        i = 0
        for name, h2_of in EDGES:
            for odd in (0, 1):
                H = 2 * h2_of(R) - odd
                for W in (WIDE_W[(i + r) % 4], WIDE_W[(i + r + 1) % 4], NARROW_W[(i + r) % 3]):
                    cases.append(pytest.param(R, W, H, id=f"R{R}-h2={name}-{'odd' if odd else 'even'}-{W}x{H}"))
                i += 1
    return cases


# The two-level kernels (k_fwd2_level_w / k_inv2_level_w<int>) take planes with W % 4 == 0 and H % 4 == 0 whose half-size
# plane is still above the LDS tail (a side > 64: every width here); a strip makes M row pairs of the coarser level,
# m0 .. min(m0 + M, h4) - 1 of h4 = H / 4.  The forward kernel runs one strip per block row (its waves sit side by side),
# the inverse int32 kernel stacks WAVES = 4 strips per block.  A pair needs its levels to exist: the forward one two
# (H >= 16: h4 >= 4), the inverse one three (the root's step never pairs: H >= 32, h4 >= 8) — so for M = 2 and 4 the
# edges below that cannot occur in any picture, and the list keeps what can:
#   M-1, M, M+1     one strip cut short / exact / followed by a strip of one pair   (forward from h4 = 4, inverse from 8)
#   2M, 2M+1        two strips, and a third of one pair
#   4M-1, 4M, 4M+1  the inverse's block of four strips: cut short, exact, followed by a second block
# Widths: 192 / 196 / 388 quads-of-four = 48 / 49 / 97, around F2_OWN = 48 quads per forward wave (one wave exact, one
# quad into a second, one quad into a third); 224 / 228 / 452 = 56 / 57 / 113 quads around V2_OWN = 56 per inverse wave.
TWO_LEVEL_W = (192, 224, 196, 228, 388, 452)


def two_level_cases():
    cases = []
    for r, R in enumerate(ROWS):
        M = mpw_of(R)
        h4s = sorted({h for h in (M - 1, M, M + 1, 2 * M, 2 * M + 1, 4 * M - 1, 4 * M, 4 * M + 1) if h >= 4})
        for i, h4 in enumerate(h4s):
            for W in (TWO_LEVEL_W[(i + r) % 6], TWO_LEVEL_W[(i + r + 3) % 6]):   # one around F2_OWN, one around V2_OWN
                cases.append(pytest.param(R, W, 4 * h4, id=f"R{R}-M{M}-h4={h4}-{W}x{4 * h4}"))
    return cases


def oracle_planes(a):
    fwd = np.stack([orc.forward(p[:, :, None])[:, :, 0] for p in a])
    inv = np.stack([orc.inverse(p[:, :, None])[:, :, 0] for p in a])
    return fwd, inv


def check_int32(ctx, opts, R, W, H):
    import torch

    rng = np.random.default_rng(H * 1009 + W)
    a = rng.integers(-40000, 40000, size=(3, H, W), dtype=np.int32)
    fwd_want, inv_want = oracle_planes(a)
    t = torch.from_numpy(a).cuda()
    for no_fused in (0, 1):
        opts.set("no_fused_levels", no_fused)
        opts.set("lift_rows", 0)
        auto = ctx.transformation_fwd(t)
        opts.set("lift_rows", R)
        what = f"lift_rows {R}, no_fused_levels {no_fused}, {W}x{H}"
        pyr = ctx.transformation_fwd(t)
        assert (pyr.cpu().numpy() == fwd_want).all(), "forward differs from the oracle: " + what
        assert torch.equal(pyr, auto), "forward differs from the automatic launch shapes: " + what
        assert torch.equal(ctx.transformation_inv(pyr), t), "inverse does not restore: " + what
        # ... and of an arbitrary array (no transform's output: details as large as the LL band)
        assert (ctx.transformation_inv(t).cpu().numpy() == inv_want).all(), "inverse differs from the oracle: " + what


@pytest.mark.parametrize("R,W,H", one_level_cases())
def test_one_level_kernels_at_forced_rows(ctx, opts, R, W, H):
    """k_fwd_level_w / k_inv_level_w and the narrow k_fwd_level / k_inv_level with R row pairs per wave strip at the
    heights where a strip is cut short, exact, or followed by a strip or a block of one row pair (EDGES above)."""
    check_int32(ctx, opts, R, W, H)


@pytest.mark.parametrize("R,W,H", two_level_cases())
def test_two_level_kernels_at_forced_rows(ctx, opts, R, W, H):
    """k_fwd2_level_w / k_inv2_level_w with M = max(2, R / 8) coarse row pairs per strip (and the one-level kernels of
    the levels below with R), against the oracle and against one launch per level."""
    check_int32(ctx, opts, R, W, H)


# ---- b. the pipelines' kernels --------------------------------------------------------------------------------------

def cut(data, st):
    """A prefix that still holds the header and the root image (as tests/test_views_gpu.py's)."""
    hdr = (st.meta_bits + st.root_bits + 7) // 8 + 2
    return data[:min(len(data), hdr + (len(data) - hdr) // 3)]


def pictures(W, H, Cn, is16):
    """smooth, noise, 0 / maxval noise (the largest coefficients), vertical 0 / maxval stripes (every HL coefficient the
    same large value), flat and a slow ramp (every coefficient of a strip in one histogram bin)."""
    rng = np.random.default_rng(W * 31 + H + Cn)
    M = M16 if is16 else 255
    dt = np.uint16 if is16 else np.uint8
    y, x = np.mgrid[:H, :W]
    ramp = np.repeat((((x + y) // 8) % (M + 1))[..., None], Cn, axis=2).astype(dt)
    stripes = np.repeat(((x & 1) * M)[..., None], Cn, axis=2).astype(dt)
    flat = np.full((H, W, Cn), M * 137 // 255, dtype=dt)
    extremes = (rng.integers(0, 2, (H, W, Cn)) * M).astype(dt)
    if is16:
        return [deep.smooth_noise(W, H, Cn, M, 3), deep.noise(W, H, Cn, M, 4), extremes, stripes, flat, ramp]
    return [orc.synth(W, H, Cn, 3, 0), orc.synth(W, H, Cn, 4, 1), extremes, stripes, flat, ramp]


FLAT = 4   # its place in pictures()
_refs = {}


def pipeline_refs(W, H, Cn, is16):
    """The oracle's side of a shape, made once: pictures, streams, cut streams and what those decode to."""
    key = (W, H, Cn, is16)
    if key not in _refs:
        pics = pictures(W, H, Cn, is16)
        enc = [deep.deep_encode(p) if is16 else orc.encode(p) for p in pics]
        streams = [e[0] for e in enc]
        cuts = [cut(d, st) for d, st in enc]
        dec = (lambda d: deep.deep_decode(d, W, H, Cn, M16)) if is16 else orc.decode
        # a whole stream gives its picture back — but for the flat one, whose stream ends after the root image: the
        # reference decodes that to the root image alone, and so must the library
        whole = [dec(d) for d in streams]
        assert all(w.shape == p.shape and (w == p).all() for w, p in zip(whole[:FLAT] + whole[FLAT + 1:], pics[:FLAT] + pics[FLAT + 1:]))
        assert whole[FLAT].shape[0] < H
        _refs[key] = (pics, streams, whole, cuts, [dec(c) for c in cuts])
    return _refs[key]


def check_pipelines(ctx, W, H, Cn, is16, what):
    pics, streams, whole, cuts, cut_pics = pipeline_refs(W, H, Cn, is16)
    if is16:
        got, _ = ctx.encode16(np.stack(pics))
        back = ctx.decode16(streams, M16)
        short = ctx.decode16(cuts, M16)
    else:
        got, _ = ctx.encode(np.stack(pics))
        back = ctx.decode(streams)
        short = ctx.decode(cuts)
    for i, p in enumerate(pics):
        assert got[i] == streams[i], f"stream {i} differs from the oracle's: {what}"
        assert back[i].shape == whole[i].shape and (back[i] == whole[i]).all(), f"decode {i} is not the picture: {what}"
        assert (short[i] is None) == (cut_pics[i] is None), f"cut stream {i}: {what}"
        if cut_pics[i] is not None:
            assert short[i].shape == cut_pics[i].shape and (short[i] == cut_pics[i]).all(), f"cut stream {i} differs from the oracle's decode: {what}"


# (W, H), W % 4 == 0 and a side above 64: 128x130 and 256x132 have W % 64 == 0 (the histograms ride along with the finest
# level: w2 % 32 == 0), the others not.  h2 = 65 = 4*16 + 1 = 64 + 1; 66 with H odd (the second strip of R = 64 is two
# pairs, the last without its odd row; R = 16: a second block of one); 257 = 4*64 + 1 at 17 quads; 129 = 2*64 + 1 =
# 8*16 + 1 at 193 quads (four strips side by side; the RGB inverse's INV_QUADS = 56: four blocks).  256x132: W % 8 == 0 and
# H % 4 == 0, h4 = 33 = 4*8 + 1 — the shape whose two finest levels the decoder undoes in one pass from 16-bit bands
# (k_inv2_level_w<uint8_t> / k_inv2_level_w_rgb), M = 2 and 8.  768x272: four levels of 16-bit bands above the tail (768, 384,
# 192, 96 wide; h2 = 136, 68 = 64 + 4 = 4*16 + 4, 34, 17) — the levels below the finest read 16-bit bands with histograms
# (w2 = 192, 96) and without (48), and the decoder pairs levels 3 and 2 as well (k_inv2_level_w<int> from 16-bit bands).
PIPE_SHAPES = [(128, 130), (260, 131), (68, 514), (772, 258), (256, 132), (768, 272)]


@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("wh", PIPE_SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_pipelines_at_forced_rows(ctx, opts, wh, Cn, is16):
    """encode / decode and encode16 / decode16 with 16 and 64 row pairs per wave strip: k_fwd_pixels_w<uint8_t | Rgb8>
    with and without histograms, k_fwd_level_w<SRC_I16 | SRC_U16 | SRC_RGB16>, k_inv_level_w<uint8_t | uint16_t>,
    k_inv_level_w_rgb and the 16-bit-band k_inv2_level_w(_rgb).  Streams are the oracle's bytes, decodes the pictures,
    decodes of cut streams the oracle's."""
    W, H = wh
    for R in (16, 64):
        opts.set("lift_rows", R)
        check_pipelines(ctx, W, H, Cn, is16, f"lift_rows {R}, {W}x{H}x{Cn}")


@pytest.mark.parametrize("switch", ["no_fine16", "no_pixels16", "no_square_tiles"])
@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
def test_pipelines_at_forced_rows_on_their_other_paths(ctx, opts, Cn, is16, switch):
    """The same with the switches that send a picture through other lifting kernels: the finest ring in the int32 pyramid,
    deep pixels through widened planes, every level through the linearised copy."""
    W, H = 256, 132
    opts.set(switch, 1)
    for R in (16, 64):
        opts.set("lift_rows", R)
        check_pipelines(ctx, W, H, Cn, is16, f"{switch}, lift_rows {R}, {W}x{H}x{Cn}")


# ---- c. the automatic choice gets there ---------------------------------------------------------------------------

def fill_chip(start, floor, strips, rows):
    """lift.hip's fill_chip, restated: the expectation the batches below are sized by."""
    r = start
    while r > floor and strips * -(-rows // r) < 4096:
        r >>= 1
    return r


# (planes, W, H, no_fused_levels, forced value of the comparison run, what the finest launches reach by fill_chip's
# formula: "rpw" (both directions) or "mpw" (forward, inverse))
#   260x132: forward 2 strips of F2_OWN = 48 quads (inverse: of V2_OWN = 56) x 2048 planes x ceil(33 / 8) >= 4096: mpw 8;
#            one launch per level: 2 strips of 64 quads x 2048 x ceil(128 / 64) = 8192: rpw 64
#   8x260, 12x516: one strip x planes x ceil(192 / 64) = 6144 / ceil(320 / 64) = 5120: rpw 64 (no second level: a side < 8)
#   196x260, one launch per level: 256 planes x ceil(192 / 16) = 3072 < 4096 <= 256 x ceil(192 / 8): rpw 8;
#            1024 planes x ceil(192 / 64) = 3072 < 4096 <= 1024 x ceil(192 / 32): rpw 32
#   196x260, two levels per pass: 49 quads are two forward strips and one inverse strip, h4 = 65: 256 planes run mpw 8
#            forward (2 x 256 x 9 = 4608) and 4 inverse (256 x 9 < 4096 <= 256 x 17); 1024 planes 8 and 8
AUTO = [
    (2048, 260, 132, 0, 64, ("mpw", 8, 8)), (2048, 260, 132, 1, 64, ("rpw", 64)),
    (2048, 8, 260, 0, 64, ("rpw", 64)), (1024, 12, 516, 0, 64, ("rpw", 64)),
    (256, 196, 260, 1, 8, ("rpw", 8)), (1024, 196, 260, 1, 32, ("rpw", 32)),
    (256, 196, 260, 0, 32, ("mpw", 8, 4)), (1024, 196, 260, 0, 64, ("mpw", 8, 8)),
]
AUTO_IDS = [f"{n}x{W}x{H}-{'one' if nf else 'two'}-{r[0]}{'/'.join(map(str, r[1:]))}" for n, W, H, nf, _, r in AUTO]


def test_the_batches_below_reach_the_values_by_the_formula():
    """(no GPU needed, but it belongs to the list above: the formula says these batches run the values the list names)"""
    for n, W, H, no_fused, forced, reaches in AUTO:
        assert W % 4 == 0
        if reaches[0] == "mpw":
            assert H % 4 == 0 and not no_fused
            assert fill_chip(8, 2, -(-(W // 4) // 48) * n, H // 4) == reaches[1]    # forward: F2_OWN = 48 quads per strip
            assert fill_chip(8, 2, -(-(W // 4) // 56) * n, H // 4) == reaches[2]    # inverse: V2_OWN = 56
            assert mpw_of(forced) in reaches[1:]
        else:
            assert no_fused or min(W, H) < 16   # (a side below 16: one level, nothing to pair)
            h2 = (H + 1) // 2
            assert fill_chip(64, 4, -(-(W // 4) // 64) * n, -(-h2 // 64) * 64) == reaches[1] == forced


@pytest.mark.parametrize("n,W,H,no_fused,forced,reaches", AUTO, ids=AUTO_IDS)
def test_large_batches_take_long_strips_by_themselves(ctx, opts, n, W, H, no_fused, forced, reaches):
    """Without the switch: batches of many small planes whose fill_chip result is what `forced` gives a small one — eight
    distinct planes repeated (the kernels cannot tell), the oracle on the eight, compared on the device; and the same
    bytes as the forced run of the same planes, which ties the switch to the path production takes."""
    import torch

    rng = np.random.default_rng(n + W)
    a = rng.integers(-40000, 40000, size=(8, H, W), dtype=np.int32)
    fwd_want, inv_want = oracle_planes(a)
    t = torch.from_numpy(a).cuda().repeat(n // 8, 1, 1)
    fwd_want = torch.from_numpy(fwd_want).cuda().repeat(n // 8, 1, 1)
    inv_want = torch.from_numpy(inv_want).cuda().repeat(n // 8, 1, 1)
    opts.set("no_fused_levels", no_fused)
    pyr = ctx.transformation_fwd(t)
    assert torch.equal(pyr, fwd_want)
    back = ctx.transformation_inv(pyr)
    assert torch.equal(back, t)
    del back
    inv = ctx.transformation_inv(t)
    assert torch.equal(inv, inv_want)
    opts.set("lift_rows", forced)
    assert torch.equal(ctx.transformation_fwd(t), pyr)
    assert torch.equal(ctx.transformation_inv(t), inv)


# ---- d. refusals -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [3, 5, 128, -1])
def test_other_values_are_refused_and_nothing_is_written(ctx, opts, value):
    import torch

    import dwt_amd

    t = torch.arange(3 * 70 * 72, dtype=torch.int32, device=ctx.device).reshape(3, 70, 72)
    opts.set("lift_rows", value)
    for call in (ctx.transformation_fwd, ctx.transformation_inv):
        out = torch.full_like(t, -77)
        with pytest.raises(dwt_amd.DwtxError) as e:
            call(t, out=out)
        assert e.value.rc == -3 and "LIFT_ROWS" in str(e.value)
        ctx.sync()
        assert bool((out == -77).all())
    opts.set("lift_rows", 0)
    assert (ctx.transformation_fwd(t).cpu().numpy() == oracle_planes(t.cpu().numpy())[0]).all()
