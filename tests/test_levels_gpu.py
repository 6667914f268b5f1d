"""GPU: decodes that stop at every level, in every sink and batch mix.

A stream that ends early, or a PIXELS cap, gives the picture of widths / heights[info.level + 1], and that size alone picks
what runs after the token walk (dwt_amd/csrc/codec.hip, decode_device): the wide inverse kernels that write the pixels, the
LDS tail or the general path; one `finish` for a batch part or one per image; fused finest rings or not.  tests/levels.py
makes the batches — every cap, every level as the shortest and the longest prefix that stops there, batches that hold every
size at once, whole batches with one short stream — from shapes whose reduced sizes change family: 263x135 (general whole,
wide at 132x68), 511x259 (general whole, wide at 256x130 and 128x65, the tail from 64x33), 520x264 (wide whole, a strip edge
at 260x132, general at 130x66) and 256x256 (wide down to 128, the tail from 64).

Every comparison is exact and against the CPU oracle (orc.decode, deep.deep_decode, floats.reference), through the checkers
of tests/test_views_gpu.py and tests/test_float_gpu.py: the whole prefilled buffer is compared, so a reduced picture must
stand in its window's corner and no other sample may change."""
import ctypes as C

import numpy as np
import pytest

import deep
import floats
import levels as Lv
import orc
import test_float_gpu as F
import test_order_gpu as O
import test_planar_gpu as P
import test_step_gpu as S
import test_views_gpu as V

pytestmark = pytest.mark.gpu

M16 = Lv.M16
FULL = Lv.SHAPES[:2]     # every case list through every sink
SMALL = Lv.SHAPES[2:]    # caps, stairs and one short stream through a few
SMALL_CASES = ("cap", "stairs", "one short", "short first")
MIXED = ("stairs", "one short", "short first")   # (and "stairs capped")
GUARD = 64

depths = pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
colours = pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])


def wh_ids(wh):
    return "%dx%d" % wh


def cases_of(W, H, Cn, is16, n, names=None):
    if names is None and (W, H) in SMALL:
        names = SMALL_CASES
    return Lv.level_cases(W, H, Cn, is16, n, names)


# ---- the sinks ----------------------------------------------------------------------------------------------------------

def quad_stack(W, H, Cn, n=4):
    """Stacked windows on the quad grid whatever W is: origin, pitch and slot are multiples of 4 samples.  (Beside one another,
    as V.band and V.grid put them, windows of an odd width are W * C samples apart: off the grid, the general path at
    every size.  Here the reduced sizes of 263x135 and 511x259 that are multiples of 4 take the wide kernels.)"""
    pitch = P.up4(W * Cn) + 8
    slot = H * pitch + 12
    return V.Layout(4 + n * slot, 4, (n, H, W, Cn), (slot, pitch, Cn, 1))


def quad_nchw(W, H, n=3):
    """P.nchw with the pitch rounded up to the quad grid: planar windows the wide kernels take at every reduced size they can."""
    pitch = P.up4(W) + 8
    cs = P.up4(H * pitch + 12)
    slot = P.up4(3 * cs + 4)
    return V.Layout(4 + n * slot, 4, (n, H, W, 3), (slot, pitch, 1, cs))


# integer views: name -> (channels, layout of (W, H), what stands for the context in V.check_decode)
VIEWS = {
    "stack-gray": (1, lambda W, H: V.stack(W, H, 1), lambda c: c), "stack-rgb": (3, lambda W, H: V.stack(W, H, 3), lambda c: c),
    "band-gray": (1, lambda W, H: V.band(W, H, 1), lambda c: c), "band-rgb": (3, lambda W, H: V.band(W, H, 3), lambda c: c),
    "grid-gray": (1, lambda W, H: V.grid(W, H, 1), lambda c: c), "grid-rgb": (3, lambda W, H: V.grid(W, H, 3), lambda c: c),
    "quad-gray": (1, lambda W, H: quad_stack(W, H, 1), lambda c: c), "quad-rgb": (3, lambda W, H: quad_stack(W, H, 3), lambda c: c),
    "nchw": (3, P.nchw, lambda c: c), "chw_grid": (3, P.chw_grid, lambda c: c), "nchw-quad": (3, quad_nchw, lambda c: c),
    "nchw-8": (3, lambda W, H: P.nchw(W, H, n=8), lambda c: c),   # (three windows are too few for a batch of every size)
    # RGB of a 4-sample pixel as R, G, B and as B, G, R (the fourth sample keeps its fill), gray of a 2-sample pixel
    "rgbx": (3, lambda W, H: S.sstack(W, H, 3, 4), S.Stepped), "bgrx": (3, lambda W, H: O.bgr(S.sstack(W, H, 3, 4)), lambda c: O.Bgr(c, True)),
    "gray-step2": (1, lambda W, H: S.sstack(W, H, 1, 2), S.Stepped),
}
SMALL_VIEWS = ["grid-gray", "grid-rgb", "nchw-8"]
# float views (tests/test_float_gpu.py's LAYOUTS): gray and planar RGB take the wide float sinks, interleaved RGB the general one
FLOAT_LAYOUTS = dict(F.LAYOUTS, **{"gray-quad": (1, lambda W, H: quad_stack(W, H, 1)), "nchw-quad": (3, quad_nchw)})
FLOATS = ["gray-grid", "gray-quad", "nchw", "nchw-quad", "rgb-grid"]
SMALL_FLOATS = ["gray-grid"]


def run_view(ctx, sink, W, H, is16, cases, n=None):
    Cn, make, wrap = VIEWS[sink]
    L = make(W, H) if n is None else sized(sink, W, H, n)
    for name, rows, pixels_max in cases(Cn, L.n):
        print(sink, name)
        V.check_decode(wrap(ctx), L, W, H, Cn, is16, rows, pixels_max)


def run_float(ctx, layout, W, H, is16, kinds, cases, n=None):
    Cn, make = FLOAT_LAYOUTS[layout]
    L = make(W, H) if n is None else sized(layout, W, H, n)
    maxval = F.maxval_of(is16)
    scale, bias = floats.SETS["imagenet"](maxval)
    for name, rows, pixels_max in cases(Cn, L.n):
        for kind in kinds:
            print(layout, kind, name)
            F.check_float(ctx, L, W, H, Cn, rows, kind, maxval, scale, bias, pixels_max)


def sized(sink, W, H, n):
    """The grid, quad-grid stack and NCHW layouts with n windows (8: two decoder parts, 24: four)."""
    if sink in ("grid-gray", "grid-rgb", "gray-grid", "rgb-grid"):
        rows, cols = {8: (2, 4), 12: (3, 4), 24: (4, 6)}[n]
        return V.grid(W, H, 1 if "gray" in sink else 3, rows=rows, cols=cols)
    if sink in ("quad-gray", "quad-rgb", "gray-quad"):
        return quad_stack(W, H, 1 if "gray" in sink else 3, n=n)
    assert sink == "nchw-quad"
    return quad_nchw(W, H, n=n)


# ---- dense slots ----------------------------------------------------------------------------------------------------------

def check_dense(ctx, W, H, Cn, is16, rows, pixels_max, padded):
    """dwtx_decode_device / dwtx_decode_device16 into the slots of a prefilled buffer: the oracle's picture densely in a slot's
    first ow * oh * C samples, the fill in every other sample; level, truncated and missing[] are what the oracle reports.
    padded: slots a multiple of 4 samples apart with a guard between them (on the quad grid: reduced sizes that are
    multiples of 4 take the wide kernels), else W * H * C apart."""
    import dwt_amd

    n = len(rows)
    size = W * H * Cn
    pix_stride = P.up4(size) + 8 if padded else size
    before = V.pattern(n * pix_stride + GUARD, is16)
    want = before.copy()
    refs = [V.oracle_decode(r, W, H, Cn, is16, pixels_max) for r in rows]
    for i, ref in enumerate(refs):
        assert ref is not None, i
        want[i * pix_stride:i * pix_stride + ref.size] = ref.reshape(-1)
    streams, lens = F.upload(ctx, rows)
    out = V.to_device(ctx, before)
    infos = (dwt_amd.DecodeInfo * n)()
    args = (ctx.h, streams.data_ptr(), streams.shape[1], lens.data_ptr(), W, H, Cn, n, deep.levels_max(W, H, pixels_max), out.data_ptr(), pix_stride)
    if is16:
        rc = ctx.lib.dwtx_decode_device16(*args, M16, C.cast(infos, C.c_void_p))
    else:
        rc = ctx.lib.dwtx_decode_device(*args, C.cast(infos, C.c_void_p))
    assert rc == 0, (rc, ctx.lib.dwtx_last_error())
    ctx.sync()
    got = V.to_host(out, is16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} samples differ, first at {bad[:5]} (slots {pix_stride} apart, pictures {[r.shape for r in refs]})"
    for i, (I, r) in enumerate(zip(infos, rows)):
        _, level, missing, _ = orc.decode_stage(r, W, H, Cn, pixels_max)
        assert I.status == 0 and I.level == level and list(I.missing) == missing.tolist(), (i, I.status, I.level, level)
        assert (I.truncated & 1) == int(missing.any()), (i, I.truncated)   # the walk stopped early: some plane is missing
        assert refs[i].shape[:2] == Lv.sizes(W, H)[level + 1][::-1], i


@pytest.mark.parametrize("n", [1, 8])
@depths
@colours
@pytest.mark.parametrize("wh", Lv.SHAPES, ids=wh_ids)
def test_dense_slots_hold_the_reduced_picture_and_the_fill(ctx, wh, Cn, is16, n):
    W, H = wh
    for name, rows, pixels_max in cases_of(W, H, Cn, is16, n):
        print(name)
        check_dense(ctx, W, H, Cn, is16, rows, pixels_max, padded=n > 1)


@depths
@colours
@pytest.mark.parametrize("wh", Lv.SHAPES, ids=wh_ids)
def test_host_decode_of_a_batch_of_every_size(ctx, wh, Cn, is16):
    """dwtx_decode_images / dwtx_decode_images16 on the "stairs" batch: outW, outH and the pixels per image."""
    W, H = wh
    for name, rows, pixels_max in cases_of(W, H, Cn, is16, 8, ("stairs",)):
        print(name)
        outs = ctx.decode16(rows, M16, pixels_max) if is16 else ctx.decode(rows, pixels_max)
        for i, (o, r) in enumerate(zip(outs, rows)):
            ref = V.oracle_decode(r, W, H, Cn, is16, pixels_max)
            assert o is not None and o.shape == ref.shape and (o == ref).all(), (name, i, None if o is None else o.shape, ref.shape)


# ---- views ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sink", list(VIEWS))
@depths
@pytest.mark.parametrize("wh", FULL, ids=wh_ids)
def test_views_hold_the_reduced_picture_in_the_corner(ctx, wh, is16, sink):
    W, H = wh
    run_view(ctx, sink, W, H, is16, lambda Cn, n: cases_of(W, H, Cn, is16, n))


@pytest.mark.parametrize("sink", SMALL_VIEWS)
@depths
@pytest.mark.parametrize("wh", SMALL, ids=wh_ids)
def test_views_of_wide_pictures_reduced(ctx, wh, is16, sink):
    W, H = wh
    run_view(ctx, sink, W, H, is16, lambda Cn, n: cases_of(W, H, Cn, is16, n))


@pytest.mark.parametrize("kind", floats.KINDS)
@pytest.mark.parametrize("layout", FLOATS)
@depths
@pytest.mark.parametrize("wh", FULL, ids=wh_ids)
def test_float_views_hold_the_reduced_picture_in_the_corner(ctx, wh, is16, layout, kind):
    """Bit patterns, with a scale and a bias per colour: cut streams make the clamps act before the conversion."""
    W, H = wh
    run_float(ctx, layout, W, H, is16, [kind], lambda Cn, n: cases_of(W, H, Cn, is16, n))


@pytest.mark.parametrize("kind", floats.KINDS)
@pytest.mark.parametrize("layout", SMALL_FLOATS)
@depths
@pytest.mark.parametrize("wh", SMALL, ids=wh_ids)
def test_float_views_of_wide_pictures_reduced(ctx, wh, is16, layout, kind):
    W, H = wh
    run_float(ctx, layout, W, H, is16, [kind], lambda Cn, n: cases_of(W, H, Cn, is16, n))


# ---- strips: 520x264 at 16 and 64 row pairs per wave ------------------------------------------------------------------------

@pytest.mark.parametrize("rows_per_wave", [16, 64])
@depths
def test_reduced_sizes_at_the_strip_edges(ctx, opts, is16, rows_per_wave):
    """260x132 is one lane into a second strip, 130x66 general; the strips of a reduced picture are its own."""
    W, H = 520, 264
    opts.set("lift_rows", rows_per_wave)
    for Cn in (1, 3):
        for name, rows, pixels_max in cases_of(W, H, Cn, is16, 8):
            print("dense", Cn, name)
            check_dense(ctx, W, H, Cn, is16, rows, pixels_max, padded=True)
    for sink in SMALL_VIEWS:
        run_view(ctx, sink, W, H, is16, lambda Cn, n: cases_of(W, H, Cn, is16, n))
    run_float(ctx, "gray-grid", W, H, is16, floats.KINDS, lambda Cn, n: cases_of(W, H, Cn, is16, n))


# ---- batches of every size: two and four decoder parts, the diagnostic switches -----------------------------------------------

PART_SINKS = ["grid-gray", "grid-rgb", "quad-gray", "nchw-quad"]


def run_mixed(ctx, W, H, is16, n, names):
    """The mixed batches through dense slots, the integer grids, the quad-grid stack and NCHW, and float32 gray, n windows each."""
    for Cn in (1, 3):
        for name, rows, pixels_max in cases_of(W, H, Cn, is16, n, names):
            print("dense", Cn, name)
            check_dense(ctx, W, H, Cn, is16, rows, pixels_max, padded=True)
    for sink in PART_SINKS:
        run_view(ctx, sink, W, H, is16, lambda Cn, m: cases_of(W, H, Cn, is16, m, names), n)
    for layout in ("gray-grid", "gray-quad"):
        run_float(ctx, layout, W, H, is16, ["float32"], lambda Cn, m: cases_of(W, H, Cn, is16, m, names), n)


@pytest.mark.parametrize("n", [8, 24])
@depths
@pytest.mark.parametrize("wh", Lv.SHAPES, ids=wh_ids)
def test_stairs_in_two_and_four_parts(ctx, wh, is16, n):
    """Every size in one batch: 8 streams are two decoder parts, 24 are four, and none of them is uniform."""
    W, H = wh
    assert len(deep.decoder_parts(n)) == (2 if n == 8 else 4)
    run_mixed(ctx, W, H, is16, n, ("stairs",))


@depths
@pytest.mark.parametrize("wh", FULL, ids=wh_ids)
def test_uniform_parts_that_start_at_an_odd_image(ctx, wh, is16):
    """Six streams are two parts of three: the second starts at image 3, whose planes in the decoder's scratch start on an odd
    int when W * H is odd.  Uniform caps and stops finish such a part in one go, through the wide kernels at 132x68, 256x130
    and 128x65 — which read the reduced pyramid 8 and 16 bytes at a time (the call once failed with DWTX_ERR_ARG there, as
    did every image-by-image finish of an odd image)."""
    W, H = wh
    assert (W * H) % 2 == 1 and [p[0] for p in deep.decoder_parts(6)] == [0, 3]
    uniform = ("cap", "stop")
    for Cn in (1, 3):
        for name, rows, pixels_max in cases_of(W, H, Cn, is16, 6, uniform):
            print("dense", Cn, name)
            check_dense(ctx, W, H, Cn, is16, rows, pixels_max, padded=True)
    for sink in ("quad-gray", "quad-rgb", "nchw-quad"):
        run_view(ctx, sink, W, H, is16, lambda Cn, m: cases_of(W, H, Cn, is16, m, uniform), 6)
    run_float(ctx, "gray-quad", W, H, is16, ["float32"], lambda Cn, m: cases_of(W, H, Cn, is16, m, uniform), 6)


@pytest.mark.parametrize("parts", [2, 4])
@depths
@pytest.mark.parametrize("wh", Lv.SHAPES, ids=wh_ids)
def test_one_short_stream_in_a_part(ctx, opts, wh, is16, parts):
    """All streams whole but one, as the last and as the first of the batch: its part loses the fused levels and the 16-bit
    rings, the others keep them (decode_parts 0, the default, runs in the tests above)."""
    W, H = wh
    opts.set("decode_parts", parts)
    run_mixed(ctx, W, H, is16, 12, ("one short", "short first"))


SWITCHES = [pytest.param(name, is16, id="%s-%s" % (name, "u16" if is16 else "u8"))
            for name in ("no_square_tiles", "no_fine16", "no_fused_levels", "no_pixels16") for is16 in (False, True) if is16 or name != "no_pixels16"]


@pytest.mark.parametrize("name,is16", SWITCHES)
@pytest.mark.parametrize("wh", Lv.SHAPES, ids=wh_ids)
def test_mixed_batches_under_the_switches(ctx, opts, wh, name, is16):
    """The paths the diagnostic switches choose between give the same pictures."""
    W, H = wh
    opts.set(name, 1)
    run_mixed(ctx, W, H, is16, 12, MIXED)
