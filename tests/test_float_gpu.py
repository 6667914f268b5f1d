"""GPU: float destinations — dwtx_decode_view_float (include/dwtx.h): streams decoded straight into float32, float16 and
bfloat16 views, `v * scale + bias` per colour.

The yardstick is the oracle's decode on the CPU (tests/test_views_gpu.py's oracle_decode: orc.decode, or tests/deep.py's for
maxval 4095) through tests/floats.py — numpy for float32, torch on the CPU for the half types — and never the library's
own integer decode.  Every comparison is of BIT PATTERNS, over the whole prefilled buffer: the windows hold the
reference's bits, every other sample its fill, which holds NaNs and infinities among everything else.  Layouts, shapes and
stream cases are those of tests/test_views_gpu.py, test_planar_gpu.py and test_step_gpu.py, counted in float samples: a
view is on the quad grid when its origin and strides are multiples of 4 SAMPLES of its own type (16 bytes of float32, 8 of
the half types) — gray and planar RGB views are then written by the inverse transform's last level, everything else by
the general conversion, and both must give the same bits."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import deep
import far
import floats
import orc
import test_planar_gpu as P
import test_step_gpu as S
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
M16 = V.M16
KINDS = floats.KINDS
STRIP_EDGES = P.STRIP_EDGES


def maxval_of(is16):
    return M16 if is16 else 255


def upload(ctx, rows):
    import torch

    stride = (max(len(r) for r in rows) + 64 + 7) // 8 * 8
    host = np.full((len(rows), stride), 0xA5, dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return torch.from_numpy(host).to(ctx.device), torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)


def check_float(ctx, L, W, H, Cn, rows, kind, maxval, scale, bias, pixels_max=-1, stepped=False, order="rgb", refs=None):
    """rows: one stream per window of layout L (counted in samples of `kind`).  The whole buffer afterwards, as bits: the
    reference in each window's corner, the fill everywhere else.  refs: the integer pictures, where they are not
    V.oracle_decode's (None: nothing is written for that row).  -> the buffer's bits."""
    assert len(rows) == L.n
    if refs is None:
        refs = [V.oracle_decode(data, W, H, Cn, maxval != 255, pixels_max) for data in rows]
    buf = floats.fill_bits(L.samples, kind)
    want = buf.copy()
    for w, ref in zip(L.np_windows(want), refs):
        if ref is not None:
            w[:ref.shape[0], :ref.shape[1]] = floats.reference(ref, kind, scale, bias, order)
    streams, lens = upload(ctx, rows)
    tf, raw = floats.to_device_floats(ctx.device, buf, kind)
    infos = ctx.decode_view_float(streams, lens, L.t_view(tf), maxval=maxval, scale=scale, bias=bias,
                                  levels_max=deep.levels_max(W, H, pixels_max), stepped=stepped, order=order)
    assert all((I.status == 0) == (ref is not None) for I, ref in zip(infos, refs))
    got = floats.bits_of(raw)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{kind}: {bad.size} samples differ, first at {bad[:5]} of {L.samples} (view offset {L.off}, strides {L.strides}): "
                           f"got {[hex(int(x)) for x in got[bad[:5]]]}, want {[hex(int(x)) for x in want[bad[:5]]]}")
    return got


def sets_for(case, maxval):
    """the scale / bias sets a stream case runs with: the per-colour one always, the identity for whole and cut streams"""
    names = ["imagenet"] + (["identity"] if case in ("whole", "cut") else [])
    return [(n,) + floats.SETS[n](maxval) for n in names]


# gray and interleaved RGB in the layouts of test_views_gpu.py, planar RGB in those of test_planar_gpu.py: name -> (channels, maker)
LAYOUTS = {"gray-stack": (1, lambda W, H: V.stack(W, H, 1)), "gray-band": (1, lambda W, H: V.band(W, H, 1)), "gray-grid": (1, lambda W, H: V.grid(W, H, 1)),
           "rgb-stack": (3, lambda W, H: V.stack(W, H, 3)), "rgb-band": (3, lambda W, H: V.band(W, H, 3)), "rgb-grid": (3, lambda W, H: V.grid(W, H, 3)),
           "nchw": (3, P.nchw), "chw_grid": (3, P.chw_grid), "cnhw": (3, P.cnhw)}
# the layouts whose views the wide sinks take at the wide shapes: gray and planar, on the quad grid of their samples
ON_GRID = ["gray-band", "gray-grid", "nchw", "chw_grid", "cnhw"]
depths = pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
wide_shapes = pytest.mark.parametrize("wh", V.WIDE, ids=lambda wh: "%dx%d" % wh)


def on_the_quad_grid(L):
    planar = L.strides[-2] == 1 and L.shape[-1] == 3
    return L.off % 4 == 0 and all(s % 4 == 0 for s in L.strides[:-2] + ((L.strides[-1],) if planar else ()))


def test_the_wide_layouts_are_on_the_quad_grid_of_any_sample():
    for name in ON_GRID:
        assert on_the_quad_grid(LAYOUTS[name][1](72, 68)), name
    assert not on_the_quad_grid(V.stack(72, 68, 1))   # (its pitch is odd: the general conversion at every shape)


# ---- 1. gray and RGB, the three types, every layout ------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(LAYOUTS))
@depths
@pytest.mark.parametrize("wh", V.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_float_decode_writes_the_windows_and_nothing_else(ctx, wh, is16, layout):
    """Whole, cut, mixed and level-capped streams (cut ones make the clamps act before the conversion) into every layout, in
    the three types: 8-bit streams with maxval 255, deep ones with 4095."""
    W, H = wh
    Cn, make = LAYOUTS[layout]
    L = make(W, H)
    for case, rows, pixels_max in V.decode_cases(W, H, Cn, is16, L.n):
        for kind in KINDS:
            for name, scale, bias in sets_for(case, maxval_of(is16)):
                print(case, kind, name)
                check_float(ctx, L, W, H, Cn, rows, kind, maxval_of(is16), scale, bias, pixels_max)


@pytest.mark.parametrize("layout", ["gray-grid", "nchw"])
@depths
@pytest.mark.parametrize("wh", STRIP_EDGES, ids=lambda wh: "%dx%d" % wh)
def test_float_sinks_at_the_strip_edges(ctx, opts, wh, is16, layout):
    """The wide sinks where a strip ends: one lane into a second strip (260), a last row pair without its odd row (131, 514
    under 16 and 64 row pairs per wave)."""
    W, H = wh
    Cn, make = LAYOUTS[layout]
    L = make(W, H)
    assert on_the_quad_grid(L)
    scale, bias = floats.SETS["imagenet"](maxval_of(is16))
    for rows_per_wave in (0, 16, 64):
        opts.set("lift_rows", rows_per_wave)
        for case, rows, pixels_max in V.decode_cases(W, H, Cn, is16, L.n)[::2]:   # whole, mixed
            for kind in KINDS:
                check_float(ctx, L, W, H, Cn, rows, kind, maxval_of(is16), scale, bias, pixels_max)


# ---- 2. off the quad grid: the general path, the same bits -----------------------------------------------------------------

@pytest.mark.parametrize("variant", ["off3", "pitch5", "csodd"])
@depths
@wide_shapes
def test_float_planar_off_the_quad_grid(ctx, wh, is16, variant):
    W, H = wh
    L = P.nchw(W, H, variant)
    assert not on_the_quad_grid(L)
    scale, bias = floats.SETS["imagenet"](maxval_of(is16))
    for case, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n)[::2]:
        for kind in KINDS:
            check_float(ctx, L, W, H, 3, rows, kind, maxval_of(is16), scale, bias, pixels_max)


@pytest.mark.parametrize("variant", ["off1", "pitch"])
@depths
@wide_shapes
def test_float_gray_off_the_quad_grid(ctx, wh, is16, variant):
    W, H = wh
    L = V.grid(W, H, 1, variant)
    assert not on_the_quad_grid(L)
    scale, bias = floats.SETS["imagenet"](maxval_of(is16))
    for case, rows, pixels_max in V.decode_cases(W, H, 1, is16, L.n)[::2]:
        for kind in KINDS:
            check_float(ctx, L, W, H, 1, rows, kind, maxval_of(is16), scale, bias, pixels_max)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "planar"])
def test_the_grid_is_the_float_samples_own(ctx, kind, Cn):
    """The quad grid is counted in samples of the destination's type, not in bytes.  An origin 4 BYTES into a 16-byte
    aligned allocation is on the grid of an 8-bit view and is one float32 sample, or two half samples, in: off the grid of
    the float view, which takes the general path.  And the reverse by element count: 4 samples in is on the grid of
    every type — 8 bytes of the half types, which would be off float32's.  The same bits whichever way each of them goes."""
    W, H = 132, 100
    quad = V.grid(W, H, 1) if Cn == 1 else P.nchw(W, H)
    assert on_the_quad_grid(quad)
    scale, bias = floats.SETS["imagenet"](255)
    name, rows, pixels_max = V.decode_cases(W, H, Cn, False, quad.n)[2]
    item = 4 if kind == "float32" else 2
    seen = set()
    for more in (1, 2, 3, 4):
        L = V.Layout(quad.samples + more, quad.off + more, quad.shape, quad.strides)
        on_bytes, on_samples = (more * item) % 4 == 0, more % 4 == 0
        assert on_the_quad_grid(L) == on_samples
        seen.add((on_bytes, on_samples))
        check_float(ctx, L, W, H, Cn, rows, kind, 255, scale, bias, pixels_max)
    assert (True, False) in seen and (True, True) in seen   # on the 8-bit grid and off the float one; on both


# ---- 3. stepped and ordered -------------------------------------------------------------------------------------------------

STEP_SHAPES = [(132, 100), (64, 64), (37, 53)]   # wide, tail, general (test_step_gpu.CLASSES)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wh", STEP_SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_float_rgb_of_a_four_sample_pixel(ctx, wh, kind, order):
    """`rgba_f[..., :3]` with stepped=True: three floats of every four are written, the fourth keeps its fill; as R, G, B and
    as B, G, R, with three different scales and biases, so that a pair applied to the wrong colour shows."""
    W, H = wh
    L = S.sstack(W, H, 3, 4)
    scale, bias = floats.SETS["imagenet"](255)
    for case, rows, pixels_max in V.decode_cases(W, H, 3, False, L.n)[::2]:
        check_float(ctx, L, W, H, 3, rows, kind, 255, scale, bias, pixels_max, stepped=True, order=order)


@pytest.mark.parametrize("kind", KINDS)
def test_float_gray_with_a_pixel_step(ctx, kind):
    W, H = 132, 100
    L = S.sstack(W, H, 1, 2)
    for case, rows, pixels_max in V.decode_cases(W, H, 1, True, L.n)[::2]:
        check_float(ctx, L, W, H, 1, rows, kind, M16, 1.0 / M16, -0.5, pixels_max, stepped=True)


@pytest.mark.parametrize("layout", ["rgb-grid", "nchw", "cnhw"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wh", [(132, 100), (37, 53)], ids=lambda wh: "%dx%d" % wh)
def test_float_bgr_interleaved_and_planar(ctx, wh, kind, layout):
    """order="bgr": dense interleaved pixels (the general conversion) and planar ones (at 132x100 the wide sink, walking down
    from the R plane): the sample at the lowest address is B and carries B's scale and bias."""
    W, H = wh
    Cn, make = LAYOUTS[layout]
    L = make(W, H)
    for is16 in (False, True):
        scale, bias = floats.SETS["imagenet"](maxval_of(is16))
        for case, rows, pixels_max in V.decode_cases(W, H, 3, is16, L.n)[1:3]:   # cut, mixed
            check_float(ctx, L, W, H, 3, rows, kind, maxval_of(is16), scale, bias, pixels_max, order="bgr")


# ---- 4. under the switches ---------------------------------------------------------------------------------------------------

SWITCHES = [("no_fused_levels", 1), ("no_fine16", 1), ("no_square_tiles", 1), ("lift_rows", 4), ("lift_rows", 64), ("decode_parts", 2), ("decode_parts", 4)]


@pytest.mark.parametrize("name,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
@pytest.mark.parametrize("layout", ["gray-grid", "chw_grid"])
@wide_shapes
def test_float_under_the_switches(ctx, opts, wh, layout, name, value):
    """The code paths the diagnostic switches choose between give the same bits: with and without two-levels-per-pass
    kernels below the finest level, 16-bit ring planes (the float sinks' 16-bit-band and int32-band variants), tiles in the
    pyramid, at 4 and 64 row pairs per wave strip, with the batch cut into 2 and 4 parts."""
    W, H = wh
    Cn, make = LAYOUTS[layout]
    L = make(W, H)
    assert on_the_quad_grid(L) and L.n >= 8
    opts.set(name, value)
    for is16 in (False, True):
        scale, bias = floats.SETS["imagenet"](maxval_of(is16))
        for case, rows, pixels_max in V.decode_cases(W, H, Cn, is16, L.n)[::2]:
            for kind in KINDS:
                check_float(ctx, L, W, H, Cn, rows, kind, maxval_of(is16), scale, bias, pixels_max)


# ---- 5. foreign depth: coefficients no 8-bit picture makes, clamped at 255 ----------------------------------------------------

@pytest.mark.parametrize("batch", ["15 planes", "16 planes"])
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "planar"])
def test_float_decode_of_deep_streams_with_maxval_255(ctx, Cn, batch):
    """A 15-plane and a 16-plane stream of deep.impulses pictures (tests/test_foreign_depth_gpu.py) among 8-bit streams, into
    float32 with maxval 255: every clamp cuts.  Four windows are two decoder parts.  "15 planes": both parts stay within
    15 planes and take the 16-bit ring planes — coefficients up to 32767 through the sinks' 16-bit-band variants;
    "16 planes": the 16-plane stream keeps its part in int32 rings while the other part, with the 15-plane stream, takes
    the 16-bit ones."""
    W, H = deep.FOREIGN_WIDE[0]
    L = V.grid(W, H, 1, rows=1, cols=4) if Cn == 1 else P.nchw(W, H, n=4)
    assert on_the_quad_grid(L) and L.n == 4 and [len(p) for p in deep.decoder_parts(4)] == [2, 2]
    s15, s16 = deep.foreign_stream(W, H, Cn, 15)[0], deep.foreign_stream(W, H, Cn, 16)[0]
    eight = [orc.encode(orc.synth(W, H, Cn, 7 + i, 0))[0] for i in range(2)]
    rows = [s15, eight[0], eight[1], deep.foreign_stream(W, H, Cn, 15, 11)[0]] if batch == "15 planes" else [s16, eight[0], s15, eight[1]]
    refs = [orc.decode(r) for r in rows]
    assert all(r is not None and r.shape == (H, W, Cn) for r in refs)
    scale, bias = floats.SETS["imagenet"](255)
    got = check_float(ctx, L, W, H, Cn, rows, "float32", 255, scale, bias, refs=refs)
    assert got is not None
    for half in ("float16", "bfloat16"):
        check_float(ctx, L, W, H, Cn, rows, half, 255, scale, bias, refs=refs)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def test_bad_float_views_are_refused_with_a_text_and_nothing_is_written(ctx):
    import torch

    import dwt_amd

    W, H, n = 72, 68, 4
    FW = 4 * W + 8
    bits = floats.fill_bits((H * 2 + 8) * FW + 64, "float32")
    tf, raw = floats.to_device_floats(ctx.device, bits, "float32")
    data, _ = V.oracle_encode(W, H, 1, False, 0)
    streams, lens = upload(ctx, [data] * n)
    stride = streams.shape[1]
    infos = (dwt_amd.DecodeInfo * n)()
    p = tf.data_ptr()
    row, win = W, (H - 1) * FW + W

    def view(dev=p, sb=4, ch=1, maxval=255, cols=0, pitch=FW, istride=W, bstride=0, cs=0):
        return dwt_amd.View(dev, sb, ch, maxval, cols, pitch, istride, bstride, cs)

    def fmt(type=0, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
        return dwt_amd.FloatFormat(type, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias))

    def decode(v, f, step=0, order=0):
        return ctx.lib.dwtx_decode_view_float(ctx.h, streams.data_ptr(), stride, lens.data_ptr(), W, H, n, -1, C.byref(v) if v is not None else None,
                                              step, order, C.byref(f) if f is not None else None, C.cast(infos, C.c_void_p))

    nan, inf = float("nan"), float("inf")
    bad = {
        "no format": (view(), None, {}, b"dwtx_float_format"),
        "unknown type": (view(), fmt(type=3), {}, b"type 3"),
        "negative type": (view(), fmt(type=-1), {}, b"type -1"),
        "float32 in 2-byte samples": (view(sb=2), fmt(type=0), {}, b"sample_bytes 2 does not match"),
        "float16 in 4-byte samples": (view(), fmt(type=1), {}, b"sample_bytes 4 does not match"),
        "bfloat16 in 4-byte samples": (view(), fmt(type=2), {}, b"sample_bytes 4 does not match"),
        "float32 in bytes": (view(sb=1), fmt(), {}, b"sample_bytes 1 does not match"),
        "scale is a NaN": (view(), fmt(scale=(1.0, nan, 1.0)), {}, b"finite"),
        "scale is infinite": (view(), fmt(scale=(inf, 1.0, 1.0)), {}, b"finite"),
        "bias is a NaN": (view(), fmt(bias=(0.0, 0.0, nan)), {}, b"finite"),
        "bias is infinite": (view(), fmt(bias=(-inf, 0.0, 0.0)), {}, b"finite"),
        # everything the integer views refuse, with float strides
        "no view": (None, fmt(), {}, b"no view"),
        "channel order": (view(), fmt(), dict(order=2), b"channel order"),
        "row_pitch below a row": (view(pitch=row - 1), fmt(), {}, b"row_pitch"),
        "channels": (view(ch=2), fmt(), {}, b"channels 2"),
        "dev not aligned to the sample": (view(dev=p + 2), fmt(), {}, b"not aligned"),
        "maxval 0": (view(maxval=0), fmt(), {}, b"maxval"),
        "maxval beyond 16 bits": (view(maxval=65536), fmt(), {}, b"maxval"),
        "pixel_step below the channels": (view(ch=3, pitch=3 * FW, istride=3 * W), fmt(), dict(step=2), b"pixel_step"),
        "side by side, overlapping columns": (view(istride=row - 1), fmt(), {}, b"overlap"),
        "side by side, pitch too short for the band": (view(pitch=3 * row + row - 1, istride=row), fmt(), {}, b"overlap"),
        "stacked, slots overlap": (view(pitch=row, istride=(H - 1) * row + row - 1), fmt(), {}, b"overlap"),
        "bands overlap": (view(cols=2, bstride=row + win - 1), fmt(), {}, b"bands overlap"),
        "planes overlap": (view(ch=3, cs=win - 1, istride=3 * win), fmt(), {}, b"overlap"),
    }
    for name, (v, f, kw, text) in bad.items():
        assert decode(v, f, **kw) == ERR_ARG, name
        assert text in ctx.lib.dwtx_last_error(), (name, ctx.lib.dwtx_last_error())
    ctx.sync()
    assert (floats.bits_of(raw) == bits).all(), "a refused float view was written to"
    # the bounds themselves are fine, and so is every maxval a deep picture may have
    good = {
        "side by side, the pitch is the band": view(pitch=4 * row, istride=row),
        "bands touch": view(cols=2, bstride=row + win),
        "maxval 1": view(maxval=1),
        "maxval 65535": view(maxval=65535),
    }
    for name, v in good.items():
        assert decode(v, fmt()) == 0, (name, ctx.lib.dwtx_last_error())
    ctx.sync()
    assert (floats.bits_of(raw) != bits).any()


# ---- 7. the stream contract ----------------------------------------------------------------------------------------------------

def test_float_view_calls_run_on_the_contexts_stream():
    """As tests/test_planar_gpu.py has it: the frame's fill lands by a copy queued on the context's own stream right before
    the call, with no synchronisation in between — a call on another stream would be overwritten by it, or write first."""
    import torch

    import dwt_amd

    W, H = 132, 100
    L = P.chw_grid(W, H)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    c = dwt_amd.Context(0, stream=s.cuda_stream)
    try:
        rows = [V.oracle_encode(W, H, 3, False, i)[0] for i in range(L.n)]
        scale, bias = floats.SETS["imagenet"](255)
        for kind in KINDS:
            bits = floats.fill_bits(L.samples, kind)
            want = bits.copy()
            for w, data in zip(L.np_windows(want), rows):
                w[...] = floats.reference(V.oracle_decode(data, W, H, 3, False), kind, scale, bias)
            pinned = torch.from_numpy(bits.view(np.int32 if kind == "float32" else np.int16)).pin_memory()
            with torch.cuda.stream(s):
                streams, lens = upload(c, rows)
                raw = torch.zeros(L.samples, dtype=pinned.dtype, device=dev)
                raw.copy_(pinned, non_blocking=True)
                c.decode_view_float(streams, lens, L.t_view(raw.view(floats.torch_dtype(kind))), scale=scale, bias=bias)
                s.synchronize()
                assert (floats.bits_of(raw) == want).all(), kind
    finally:
        c.close()


# ---- 8. one far case ------------------------------------------------------------------------------------------------------------

FAR_FILL = 0x7FC0A5A5   # a quiet NaN with a payload (positive as torch's int32 holds it): no decode writes it
# GiB measured on an MI355X (free memory before the test minus the lowest seen during it), GiB below which the test skips:
# measured * 1.25, rounded up — the rule of tests/test_far_gpu.py
FAR_NEED_GIB = (25.02, 32)


@contextlib.contextmanager
def far_float_context():
    import torch

    import dwt_amd
    import test_far_gpu as FG

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.empty_cache()
    need, free = FAR_NEED_GIB[1], torch.cuda.mem_get_info()[0]
    if free < need * 2**30:
        pytest.skip(f"needs about {need} GiB of free HBM ({free / 2**30:.1f} GiB free)")
    peak = FG.Peak("far-row-gray-float32")
    c = dwt_amd.Context(0)
    try:
        yield c, peak
        peak.look()
        peak.report()
    except dwt_amd.DwtxError as e:
        if e.rc == -4:   # DWTX_ERR_DEVICE: nothing more is started on a device that may have faulted
            pytest.exit(f"far float rows: the device reported an error, the session ends here: {e}", returncode=3)
        raise
    finally:
        c.close()
        torch.cuda.empty_cache()


def test_far_rows_of_a_float32_gray_window():
    """tests/far.py's far-row layout in float32 samples: two 132x68 gray windows side by side whose rows are 2^26 + 12
    samples apart — row 32 starts more than 2^31 samples (2^33 bytes) from dev, row 64 more than 2^32 — in a frame that
    begins 2^31 samples before the view, so that a row offset formed in 32 bits lands on frame.  The wide float32 sink
    writes them; afterwards the windows hold the reference's bits and, once they hold the fill again, nothing else in the
    whole frame has changed."""
    import torch

    import test_far_gpu as FG

    W, H = far.WIDE_A
    L = far._far_row(far.WIDE_A, 1, 0)
    assert on_the_quad_grid(L) and L.strides[1] * 32 > far.T31 and L.strides[1] * 64 > far.T32 and L.strides[1] < far.T31
    scale, bias = floats.SETS["imagenet"](255)
    fill = FAR_FILL
    with far_float_context() as (c, peak):
        frame = torch.empty(L.samples, dtype=torch.int32, device=c.device)
        frame.fill_(fill)
        tv = L.t_view(frame.view(torch.float32))
        iv = L.t_view(frame)
        for case, rows, pixels_max in V.decode_cases(W, H, 1, False, L.n)[::2]:   # whole, mixed
            streams, lens = upload(c, rows)
            c.decode_view_float(streams, lens, tv, scale=scale, bias=bias, levels_max=deep.levels_max(W, H, pixels_max))
            peak.look()
            wrong = []
            for i, data in enumerate(rows):
                ref = V.oracle_decode(data, W, H, 1, False, pixels_max)
                oh, ow = ref.shape[:2]
                got = iv[i, :oh, :ow].contiguous().cpu().numpy().view(np.uint32)
                if not (got == floats.reference(ref, "float32", scale, bias)).all():
                    wrong.append((case, i))
                iv[i, :oh, :ow] = fill
            bad = FG.strays(frame, fill)
            assert not wrong, f"windows differ from the reference: {wrong}; stray samples at {bad}"
            assert not bad, f"samples outside the written rectangles changed, first at {bad}"
        del frame, tv, iv
