"""GPU parity: colour transform + multi-level CDF 5/3 through the C ABI vs the oracle."""
import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 1), (8, 9, 3), (9, 8, 1), (15, 15, 3), (16, 16, 1), (53, 37, 3), (77, 131, 3), (300, 17, 1),
          (17, 300, 3), (255, 257, 1), (257, 255, 3), (64, 64, 3), (240, 320, 3), (129, 1000, 1), (1080, 1920, 3),
          (540, 9, 1)]


def to_planes(a):
    """[H,W,C] interleaved -> [C,H,W]"""
    return np.ascontiguousarray(np.moveaxis(a, 2, 0))


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_oracle(ctx, shape):
    import torch

    H, W, Cn = shape
    pix = orc.synth(W, H, Cn, 3, 0)
    coef, _, _ = orc.stage_dump(pix)
    t = torch.from_numpy(pix[None]).cuda()
    planes = ctx.planes_from_pixels(t)
    pyr = ctx.transformation_fwd(planes)
    got = pyr.cpu().numpy()
    assert (got == to_planes(coef)).all()
    back = ctx.transformation_inv(pyr)
    assert torch.equal(back, planes)
    out = ctx.pixels_from_planes(back, Cn)
    assert (out.cpu().numpy()[0] == pix).all()


@pytest.mark.parametrize("shape", [(8, 8), (33, 71), (128, 96), (511, 513)])
def test_random_int_planes_batch(ctx, shape):
    """Batch of planes with full-range-ish ints: forward equals the oracle, inverse restores."""
    import torch

    H, W = shape
    rng = np.random.default_rng(5)
    P = 5
    a = rng.integers(-5000, 5000, size=(P, H, W), dtype=np.int32)
    want = np.stack([orc.forward(a[p][:, :, None])[:, :, 0] for p in range(P)])
    pyr = ctx.transformation_fwd(torch.from_numpy(a).cuda())
    assert (pyr.cpu().numpy() == want).all()
    back = ctx.transformation_inv(pyr)
    assert (back.cpu().numpy() == a).all()
    # inverse of an arbitrary (non-transform) pyramid also matches the oracle
    inv_want = np.stack([orc.inverse(a[p][:, :, None])[:, :, 0] for p in range(P)])
    inv_got = ctx.transformation_inv(torch.from_numpy(a).cuda())
    assert (inv_got.cpu().numpy() == inv_want).all()


@pytest.mark.parametrize("shape", [(200, 4), (333, 8), (131, 12), (65, 256), (66, 260), (67, 516), (257, 1028), (1030, 68), (2050, 72), (3, 128), (2, 512)])
def test_wide_kernels_at_their_edges(ctx, shape):
    """The 16-byte-per-lane kernels work in batches of two row pairs with loads from clamped places (lift.hip): one quad
    per row, one lane past a full strip, odd heights (the last row pair has no odd row), strips that end inside a batch,
    heights of two and three rows.  int32 planes both ways against the oracle, and 8-bit pixels through the codec."""
    import torch

    H, W = shape
    rng = np.random.default_rng(H * 7 + W)
    a = rng.integers(-3000, 3000, size=(3, H, W), dtype=np.int32)
    want = np.stack([orc.forward(a[p][:, :, None])[:, :, 0] for p in range(3)])
    pyr = ctx.transformation_fwd(torch.from_numpy(a).cuda())
    assert (pyr.cpu().numpy() == want).all()
    inv_want = np.stack([orc.inverse(a[p][:, :, None])[:, :, 0] for p in range(3)])
    assert (ctx.transformation_inv(torch.from_numpy(a).cuda()).cpu().numpy() == inv_want).all()
    if H >= 8 and W >= 8:
        for Cn in (1, 3):
            pix = np.stack([orc.synth(W, H, Cn, 11, 1), (rng.integers(0, 2, (H, W, Cn)) * 255).astype(np.uint8)])
            streams, _ = ctx.encode(pix)
            assert streams == [orc.encode(x)[0] for x in pix]
            assert all((o == x).all() for o, x in zip(ctx.decode(streams), pix))


def test_4096_gray_roundtrip_and_checksum(ctx):
    """BASELINE config B size: round trip + checksum against the oracle's pyramid."""
    import torch

    pix = orc.synth(4096, 4096, 1, 0, 0)
    coef, _, _ = orc.stage_dump(pix)
    t = torch.from_numpy(pix[None]).cuda()
    planes = ctx.planes_from_pixels(t)
    pyr = ctx.transformation_fwd(planes)
    assert (pyr.cpu().numpy()[0] == coef[:, :, 0]).all()
    assert torch.equal(ctx.transformation_inv(pyr), planes)


def test_small_inverse_root_only(ctx):
    """decode.c quirk: a root-only decode still runs one inverse level on a <8 image."""
    import torch

    rng = np.random.default_rng(2)
    for (H, W) in [(4, 5), (5, 8), (4, 4), (7, 6)]:
        a = rng.integers(-100, 100, size=(2, H, W), dtype=np.int32)
        want = np.stack([orc.inverse(a[p][:, :, None])[:, :, 0] for p in range(2)])
        got = ctx.transformation_inv(torch.from_numpy(a).cuda())
        assert (got.cpu().numpy() == want).all()


def merge_rings(pyr, r16, mask, W, H):
    """the pyramid as one int32 array: the ring levels in `mask` come from the 16-bit planes"""
    g = orc.geometry(W, H)
    out = pyr.copy()
    for l in range(g.levels):
        if (mask >> l) & 1:
            w0, h0, w1, h1 = g.widths[l], g.heights[l], g.widths[l + 1], g.heights[l + 1]
            out[:, :h1, w0:w1] = r16[:, :h1, w0:w1]
            out[:, h0:h1, :w0] = r16[:, h0:h1, :w0]
    return out


@pytest.mark.parametrize("shape", [(128, 128, 1), (96, 260, 3), (1080, 1920, 3), (67, 516, 1), (1024, 1024, 1), (540, 72, 3), (257, 1028, 3)])
@pytest.mark.parametrize("rings16", [True, False])
def test_pixel_transforms_as_the_pipelines_run_them(ctx, shape, rings16):
    """dwtx_transformation_fwd_pixels / _inv_pixels (encode.c:155-159, decode.c:258-264 in one pass each, the finest rings
    as 16-bit values): the pyramid is the oracle's, a noise picture with the largest steps an 8-bit source can make too,
    and the inverse of the pyramid gives the pixels back."""
    import torch

    H, W, Cn = shape
    rng = np.random.default_rng(W + H)
    pix = np.stack([orc.synth(W, H, Cn, 4, 0), orc.synth(W, H, Cn, 5, 1), (rng.integers(0, 2, (H, W, Cn)) * 255).astype(np.uint8)])
    t = torch.from_numpy(pix).cuda()
    pyr, r16, mask = ctx.transformation_fwd_pixels(t, rings16=rings16)
    assert rings16 or mask == 0
    got = merge_rings(pyr.cpu().numpy(), r16.cpu().numpy() if r16 is not None else None, mask, W, H)
    want = np.concatenate([to_planes(orc.stage_dump(p)[0]) for p in pix])
    assert (got == want).all()
    back = ctx.transformation_inv_pixels(pyr, r16, mask, Cn)
    assert torch.equal(back, t)


def ring_bands(g, l):
    """(rows, columns) of the three detail bands of ring level l in a pyramid plane: HL, LH, HH"""
    w0, h0, w1, h1 = g.widths[l], g.heights[l], g.widths[l + 1], g.heights[l + 1]
    return [((0, h0), (w0, w1)), ((h0, h1), (0, w0)), ((h0, h1), (w0, w1))]


def arbitrary_pyramid(rng, P, H, W, Cn, mask):
    """-> (int32 pyramid [P,H,W], int16 ring planes [P,H,W] or None, the merged pyramid): coefficients no transform made.
    Uniform in +-150 (gray, Y) or +-400 (Co, Cg) with one in two thousand anywhere in +-2^20 (int32) or in all of int16 (the ring levels in `mask`, which
    the int32 array then does not hold: it has a sentinel there), 128 added to the root band of gray / Y — so that about half
    of the inverse's samples fall inside [0, 255] and the rest leave it on either side.  Every band of a 16-bit ring has
    -32768 and 32767 in its corners and in the middle of its first and last row and column."""
    g = orc.geometry(W, H)
    amp = np.array([150 if p % Cn == 0 else 400 for p in range(P)], dtype=np.int32)[:, None, None]   # gray / Y; Co, Cg
    pyr = rng.integers(-1000, 1001, size=(P, H, W), dtype=np.int32) * amp // 1000
    rare = rng.random((P, H, W)) < 0.0005
    pyr[rare] = rng.integers(-(1 << 20), (1 << 20) + 1, size=int(rare.sum()), dtype=np.int32)
    pyr[::Cn, :g.heights[0], :g.widths[0]] += 128
    if not mask:
        return pyr, None, pyr
    r16 = (rng.integers(-1000, 1001, size=(P, H, W), dtype=np.int32) * amp // 1000).astype(np.int16)
    r16[rare] = rng.integers(-32768, 32768, size=int(rare.sum()), dtype=np.int16)
    for l in range(g.levels):
        if (mask >> l) & 1:
            for k, ((y0, y1), (x0, x1)) in enumerate(ring_bands(g, l)):
                pyr[:, y0:y1, x0:x1] = -(1 << 30)   # not read
                ys, xs = (y0, (y0 + y1) // 2, y1 - 1), (x0, (x0 + x1) // 2, x1 - 1)
                edge = [(y, x) for y in ys for x in xs if y != ys[1] or x != xs[1]]
                for i, (y, x) in enumerate(edge):
                    r16[:, y, x] = 32767 if (i + k) & 1 else -32768
    return pyr, r16, merge_rings(pyr, r16, mask, W, H)


def popcount(v):
    return bin(v).count("1")


INV_PIXELS_SHAPES = [(72, 132, 1), (72, 132, 3), (260, 516, 1), (260, 516, 3), (1024, 1024, 1), (320, 1088, 1), (320, 1088, 3)]


@pytest.mark.parametrize("shape", INV_PIXELS_SHAPES)
@pytest.mark.parametrize("rings16", [False, True], ids=["int32", "rings16"])
def test_inverse_to_8_bit_pixels_of_arbitrary_pyramids(ctx, shape, rings16):
    """dwtx_transformation_inv_pixels on pyramids that no 8-bit picture makes: the clamps of the fused kernels (image.h:39-51,
    pnm.h:108 — Y to [0,255], Co and Cg to [-255,255], then R, G, B to [0,255]) cut about half of the samples, which the
    test asserts of its own input, and the 16-bit rings hold all of int16.  72x132: one wide level above the LDS tail;
    1024x1024: four 16-bit ring levels, two two-level passes; 320x1088: five of its six ring levels are 16-bit, so
    k_inv2_level_w* reads 16-bit rings on both of its levels and the step below them an int32 ring.  Everything in int32
    (no ring planes) and with the rings of the reported mask in int16; against orc.inverse of the merged pyramid and numpy's
    colour transform and clamps."""
    import torch

    H, W, Cn = shape
    n = 2
    g = orc.geometry(W, H)
    reported = ctx.transformation_fwd_pixels(torch.zeros((1, H, W, Cn), dtype=torch.uint8, device=ctx.device))[2]
    assert reported & (1 << (g.levels - 1))
    assert popcount(reported) == {1024: 4, 1088: 5}.get(W, 1)
    if W == 1088:
        assert g.levels == 6 and not reported & 1   # ring level 0 stays int32: the boundary is inside the picture
    mask = reported if rings16 else 0
    pyr, r16, merged = arbitrary_pyramid(np.random.default_rng(H + W + Cn), n * Cn, H, W, Cn, mask)
    assert np.abs(merged).max() <= 1 << 20
    if rings16:
        assert r16.min() == -32768 and r16.max() == 32767
    inv = [orc.inverse(np.moveaxis(merged[i * Cn:(i + 1) * Cn], 0, 2)) for i in range(n)]
    for a in inv:
        print(shape, "mask 0x%x" % mask, "inside, outside:", deep.clamp_shares(a, Cn))
        assert deep.clamps_are_at_work(a, Cn)
    want = np.stack([deep.ycocg2rgb(a, 255) if Cn == 3 else np.clip(a, 0, 255) for a in inv]).astype(np.uint8)
    got = ctx.transformation_inv_pixels(torch.from_numpy(pyr).to(ctx.device), torch.from_numpy(r16).to(ctx.device) if rings16 else None,
                                        mask, Cn)
    assert (got.cpu().numpy() == want).all()


@pytest.mark.parametrize("shape", [(53, 37, 1), (77, 131, 3), (100, 258, 3), (66, 1030, 1), (9, 10, 3)])
def test_8_bit_pixels_from_planes_that_the_clamps_cut(ctx, shape):
    """dwtx_pixels_from_planes (k_pixels_from_planes<uint8_t>) on planes in about +-2000, widths that are no multiple of 4:
    most of gray / Y in [-150, 400] and of Co, Cg in [-400, 400], one sample in seven anywhere in +-2000."""
    import torch

    H, W, Cn = shape
    n = 2
    rng = np.random.default_rng(H * W + Cn)
    a = rng.integers(-400, 401, size=(n, H, W, Cn), dtype=np.int32)
    a[..., 0] = rng.integers(-150, 401, size=(n, H, W), dtype=np.int32)
    far = rng.random(a.shape) < 1 / 7
    a[far] = rng.integers(-2000, 2001, size=int(far.sum()), dtype=np.int32)
    assert W % 4 != 0
    for img in a:
        print(shape, "inside, outside:", deep.clamp_shares(img, Cn))
        assert deep.clamps_are_at_work(img, Cn)
    want = np.stack([deep.ycocg2rgb(img, 255) if Cn == 3 else np.clip(img, 0, 255) for img in a]).astype(np.uint8)
    planes = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)).reshape(n * Cn, H, W)).to(ctx.device)
    assert (ctx.pixels_from_planes(planes, Cn).cpu().numpy() == want).all()


def test_pixel_transforms_refuse_shapes_their_kernels_do_not_take(ctx):
    import torch

    for H, W in ((100, 131), (64, 64), (40, 40)):
        t = torch.zeros((1, H, W, 1), dtype=torch.uint8, device=ctx.device)
        with pytest.raises(RuntimeError):
            ctx.transformation_fwd_pixels(t)


@pytest.mark.parametrize("shape", [(68, 244), (132, 248), (260, 488), (516, 492), (72, 976), (128, 980), (388, 1220), (1080, 1920), (2048, 2048),
                                   (68, 68), (512, 4), (260, 8), (1028, 260), (68, 192), (132, 196), (260, 224), (516, 228), (1040, 448), (76, 452),
                                   (4096, 96), (644, 3588), (132, 388)])
def test_two_levels_per_pass_equal_one_launch_per_level(ctx, shape, opts):
    """k_fwd2_level_w / k_inv2_level_w (two levels of cdf53.h:9-61 / encode.c:16-30, decode.c:16-30 in one pass, the LL band between them never in memory):
    widths around whole numbers of the waves' strips — F2_OWN = 48 quads forward (192, 196, 388: one strip, one quad into a
    second, one quad into a third), V2_OWN = 56 quads inverse (224, 228, 448, 452) —, heights that end strips inside / at the
    end of a row pair of the coarser level, the smallest shapes it takes — against the oracle, and the same bytes as one
    launch per level."""
    import torch

    H, W = shape
    rng = np.random.default_rng(H + 3 * W)
    a = rng.integers(-40000, 40000, size=(3, H, W), dtype=np.int32)
    want = np.stack([orc.forward(a[p][:, :, None])[:, :, 0] for p in range(3)])
    t = torch.from_numpy(a).cuda()
    fused = ctx.transformation_fwd(t)
    assert (fused.cpu().numpy() == want).all()
    assert torch.equal(ctx.transformation_inv(fused), t)                       # k_inv2_level_w
    inv_want = np.stack([orc.inverse(a[p][:, :, None])[:, :, 0] for p in range(3)])   # ... and of an arbitrary pyramid
    inv_fused = ctx.transformation_inv(t)
    assert (inv_fused.cpu().numpy() == inv_want).all()
    opts.set("no_fused_levels", 1)
    plain = ctx.transformation_fwd(t)
    assert torch.equal(plain, fused)
    assert torch.equal(ctx.transformation_inv(fused), t)
    assert torch.equal(ctx.transformation_inv(t), inv_fused)
