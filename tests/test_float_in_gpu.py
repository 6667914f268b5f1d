"""GPU: float sources — dwtx_encode_view_float (include/dwtx.h): float32, float16 and bfloat16 views quantised
(`rint(x * scale + bias)` per colour, two float32 roundings, clamped to [0, maxval], NaN -> 0) and coded where they lie.

The yardstick is the oracle on the integers tests/quant.py makes of the floats on the CPU: orc.encode for maxval 255,
tests/deep.py's deep_encode for 4095 — never the library's own integer encode as the only witness; its encode_device /
encode_device16 on the quantised dense copy is compared as well, records included, as tests/test_views_gpu.py does.  The
frame around the windows holds floats.fill_bits — NaNs and infinities among everything else — so that a read outside a
window changes bytes; the windows hold quant.py's pictures with their planted ties, clamped samples, infinities and NaNs.
Layouts, shapes and switches are those of tests/test_float_gpu.py, counted in float samples."""
import ctypes as C

import numpy as np
import pytest

import deep
import floats
import orc
import quant
import test_encode_index_gpu as EI
import test_float_gpu as F
import test_planar_gpu as P
import test_step_gpu as S
import test_views_gpu as V

pytestmark = pytest.mark.gpu

ERR_ARG = V.ERR_ARG
KINDS = quant.KINDS
MAXVALS = [255, V.M16]
PICS = 5   # window i holds picture i % PICS: neighbours in a row and in a column of every grid differ


def check_float_in(ctx, L, W, H, Cn, kind, maxval, set_name, capacities=(0,), stepped=False, order="rgb", first_pic=0):
    """The windows of layout L (counted in samples of `kind`) filled with quant.py's pictures, the rest with the fill:
    stream and record of every window against the oracle and against the integer encode of the quantised dense copy."""
    scale, bias = quant.SETS[set_name](maxval)
    is16 = maxval > 255
    buf = floats.fill_bits(L.samples, kind)
    ids = [(first_pic + i) % PICS for i in range(L.n)]
    wants = []
    for i, w in zip(ids, L.np_windows(buf)):
        bits, v = quant.window(W, H, Cn, kind, maxval, set_name, i, order)
        w[...] = bits
        wants.append(v)
    tf, raw = floats.to_device_floats(ctx.device, buf, kind)
    tv = L.t_view(tf)
    dense = V.to_device(ctx, np.stack(wants).astype(np.uint16 if is16 else np.uint8))
    for capacity in capacities:
        out, info = ctx.encode_view_float(tv, maxval=maxval, scale=scale, bias=bias, capacity=capacity, stepped=stepped, order=order)
        dout, dinfo = (ctx.encode_device16 if is16 else ctx.encode_device)(dense, capacity)
        infos, dinfos = V.infos_of(info), V.infos_of(dinfo)
        host, dhost = out.cpu().numpy(), dout.cpu().numpy()
        assert out.shape == dout.shape
        for k, i in enumerate(ids):
            want, st = quant.oracle_encode(W, H, Cn, kind, maxval, set_name, i, order, capacity)
            I = infos[k]
            where = (kind, maxval, set_name, order, k, capacity)
            assert I.error == 0, where
            assert host[k, :I.nbytes].tobytes() == want, where
            if capacity <= 0:   # (the zero padding after a stream that CAPACITY does not cut: include/dwtx.h, dwtx_encode_planes)
                assert not host[k, I.nbytes:min(host.shape[1], (I.nbytes + 3) // 4 * 4 + 16)].any(), where
            assert list(I.planes)[:Cn] == list(st.planes)[:Cn] and (I.root_bits, I.total_bits) == (st.root_bits, st.total_bits), where
            assert V.fields(I) == V.fields(dinfos[k]), where
            assert dhost[k, :I.nbytes].tobytes() == want, where
    assert (floats.bits_of(raw) == buf).all(), "the source was written to"


def on_the_quad_grid(L):
    return F.on_the_quad_grid(L)


# ---- 1. layouts, types and depths -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(F.LAYOUTS))
@pytest.mark.parametrize("maxval", MAXVALS)
@pytest.mark.parametrize("wh", V.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_float_encode_equals_the_oracle_on_the_quantised_windows(ctx, wh, maxval, layout):
    """Every layout in the three types and the three scale / bias sets, at capacities 0 and 500."""
    W, H = wh
    Cn, make = F.LAYOUTS[layout]
    L = make(W, H)
    for kind in KINDS:
        for name in quant.SETS:
            print(kind, name)
            check_float_in(ctx, L, W, H, Cn, kind, maxval, name, capacities=(0, 500))


@pytest.mark.parametrize("layout,kind,maxval", [("gray-grid", "float16", 255), ("chw_grid", "float32", V.M16)])
def test_float_encoder_parts_start_mid_grid(ctx, layout, kind, maxval):
    """128 windows: the encoder cuts the batch into four parts, each of which starts at its own window of the 8 x 16 grid
    and carries the format along (tests/test_views_gpu.py's and test_planar_gpu.py's test of the same name)."""
    W, H = 72, 68
    L = V.grid(W, H, 1, "quad", rows=8, cols=16) if layout == "gray-grid" else P.chw_grid(W, H, rows=8, cols=16)
    assert L.n == 128 and on_the_quad_grid(L)
    check_float_in(ctx, L, W, H, F.LAYOUTS[layout][0], kind, maxval, "imagenet_inv")


# ---- 2. strip edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["gray-grid", "nchw"])
@pytest.mark.parametrize("maxval", MAXVALS)
@pytest.mark.parametrize("wh", P.STRIP_EDGES, ids=lambda wh: "%dx%d" % wh)
def test_float_sources_at_the_strip_edges(ctx, opts, wh, maxval, layout):
    """The wide sources where a strip ends: one lane into a second strip (260), a last row pair without its odd row (131,
    514 under 16 and 64 row pairs per wave)."""
    W, H = wh
    Cn, make = F.LAYOUTS[layout]
    L = make(W, H)
    assert on_the_quad_grid(L)
    for rows_per_wave in (16, 64):
        opts.set("lift_rows", rows_per_wave)
        for kind in KINDS:
            check_float_in(ctx, L, W, H, Cn, kind, maxval, "imagenet_inv")


# ---- 3. off the quad grid: the general way, the same bytes -------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["off1", "pitch"])
@pytest.mark.parametrize("maxval", MAXVALS)
@pytest.mark.parametrize("wh", V.WIDE, ids=lambda wh: "%dx%d" % wh)
def test_float_gray_off_the_quad_grid(ctx, wh, maxval, variant):
    W, H = wh
    L = V.grid(W, H, 1, variant)
    assert not on_the_quad_grid(L)
    for kind in KINDS:
        check_float_in(ctx, L, W, H, 1, kind, maxval, "unit")


@pytest.mark.parametrize("variant", ["off3", "pitch5", "csodd"])
@pytest.mark.parametrize("maxval", MAXVALS)
@pytest.mark.parametrize("wh", V.WIDE, ids=lambda wh: "%dx%d" % wh)
def test_float_planar_off_the_quad_grid(ctx, wh, maxval, variant):
    W, H = wh
    L = P.nchw(W, H, variant)
    assert not on_the_quad_grid(L)
    for kind in KINDS:
        check_float_in(ctx, L, W, H, 3, kind, maxval, "imagenet_inv")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "planar"])
def test_the_grid_is_the_float_samples_own(ctx, kind, Cn):
    """As tests/test_float_gpu.py has it for the sinks: the quad grid is counted in samples of the source's type.  One, two
    and three samples in, a view is off it (two half samples are 4 bytes, two float32 samples 8: on a byte grid, off the
    float one); four samples in — 8 bytes of the half types — it is on it.  The same bytes whichever way each goes."""
    W, H = 132, 100
    quad = V.grid(W, H, 1) if Cn == 1 else P.nchw(W, H)
    assert on_the_quad_grid(quad)
    item = 4 if kind == "float32" else 2
    seen = set()
    for more in (1, 2, 3, 4):
        L = V.Layout(quad.samples + more, quad.off + more, quad.shape, quad.strides)
        on_bytes, on_samples = (more * item) % 4 == 0, more % 4 == 0
        assert on_the_quad_grid(L) == on_samples
        seen.add((on_bytes, on_samples))
        check_float_in(ctx, L, W, H, Cn, kind, 255, "imagenet_inv")
    assert (True, False) in seen and (True, True) in seen


# ---- 4. step and order ---------------------------------------------------------------------------------------------------------------

STEP_SHAPES = F.STEP_SHAPES   # wide, tail, general


@pytest.mark.parametrize("order", ["rgb", "bgr"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wh", STEP_SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_float_rgb_of_a_four_sample_pixel(ctx, wh, kind, order):
    """`rgba_f[..., :3]` with stepped=True: the fourth float of every pixel is the fill (a NaN, an infinity, anything) and
    is never read; as R, G, B and as B, G, R with three different scales and biases."""
    W, H = wh
    check_float_in(ctx, S.sstack(W, H, 3, 4), W, H, 3, kind, 255, "imagenet_inv", stepped=True, order=order)


@pytest.mark.parametrize("kind", KINDS)
def test_float_gray_with_a_pixel_step(ctx, kind):
    W, H = 132, 100
    check_float_in(ctx, S.sstack(W, H, 1, 2), W, H, 1, kind, V.M16, "unit", stepped=True)


@pytest.mark.parametrize("layout", ["rgb-grid", "nchw", "cnhw"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wh", [(132, 100), (37, 53)], ids=lambda wh: "%dx%d" % wh)
def test_float_bgr_interleaved_and_planar(ctx, wh, kind, layout):
    """order="bgr": dense interleaved pixels (the general way) and planar ones (at 132x100 the wide sources, walking down
    from the R plane): the sample at the lowest address is B and takes B's scale and bias."""
    W, H = wh
    Cn, make = F.LAYOUTS[layout]
    for maxval in MAXVALS:
        check_float_in(ctx, make(W, H), W, H, 3, kind, maxval, "imagenet_inv", order="bgr")


# ---- 5. under the switches --------------------------------------------------------------------------------------------------------

SWITCHES = [("no_fused_levels", 1), ("no_fine16", 1), ("no_square_tiles", 1), ("exact_orders", 1), ("no_capacity_cut", 1), ("lift_rows", 4),
            ("lift_rows", 64)]


@pytest.mark.parametrize("name,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
@pytest.mark.parametrize("layout", ["gray-grid", "chw_grid"])
@pytest.mark.parametrize("wh", V.WIDE, ids=lambda wh: "%dx%d" % wh)
def test_float_encode_under_the_switches(ctx, opts, wh, layout, name, value):
    W, H = wh
    Cn, make = F.LAYOUTS[layout]
    L = make(W, H)
    assert on_the_quad_grid(L)
    opts.set(name, value)
    for maxval in MAXVALS:
        for kind in KINDS:
            check_float_in(ctx, L, W, H, Cn, kind, maxval, "unit", capacities=(0, 500))


# ---- 6. the bit-plane limit --------------------------------------------------------------------------------------------------------

def _float_stack(ctx, pics, kind="float32"):
    """integer pictures -> (a dense float tensor [n,H,W,C] holding exactly those values, its integer twin)"""
    bits = quant.to_bits(np.stack(pics).astype(np.float64), kind)
    tf, raw = floats.to_device_floats(ctx.device, bits.reshape(-1), kind)
    return tf.view(bits.shape), raw


def test_a_picture_with_more_than_16_planes_is_refused_alone(ctx):
    """maxval 65535 on a noise picture: dev_info[i].error = 1 for it while its neighbours are coded (the pictures of
    tests/test_deep_gpu.py's refusal test, as float32 with the identity)."""
    W, H, Cn = 256, 200, 3
    pics = [deep.smooth_noise(W, H, Cn, 65535, 1), deep.noise(W, H, Cn, 65535, 2), deep.blocks(W, H, Cn, 4095, 3)]
    assert max(deep.deep_encode(pics[1])[1].planes) > 16
    tf, _ = _float_stack(ctx, pics)
    out, info = ctx.encode_view_float(tf, maxval=65535)
    infos, host = V.infos_of(info), out.cpu().numpy()
    assert [I.error for I in infos] == [0, 1, 0]
    for i in (0, 2):
        assert host[i, :infos[i].nbytes].tobytes() == deep.deep_encode(pics[i])[0], i


@pytest.mark.parametrize("kind", KINDS)
def test_maxval_4095_is_never_refused(ctx, kind):
    """Uniform noise over the whole range, the hardest picture there is: coded, to the oracle's bytes."""
    W, H, Cn = 132, 100, 3
    pics = [deep.noise(W, H, Cn, 4095, 5), deep.checker(W, H, Cn, 4095)]
    tf, raw = _float_stack(ctx, pics, kind)
    v = quant.quantise(floats.bits_of(raw).reshape(len(pics), H, W, Cn), kind, 1.0, 0.0, 4095)
    out, info = ctx.encode_view_float(tf, maxval=4095)
    infos, host = V.infos_of(info), out.cpu().numpy()
    for i in range(len(pics)):
        want, st = deep.deep_encode(v[i].astype(np.uint16))
        assert infos[i].error == 0 and max(st.planes) <= 16
        assert host[i, :infos[i].nbytes].tobytes() == want, i


@pytest.mark.parametrize("wh", [(132, 100), (37, 53)], ids=lambda wh: "%dx%d" % wh)
def test_float16_subnormals_are_kept(ctx, wh):
    """A gray float16 picture of nothing but 0, 2^-24, 2 * 2^-24 and 3 * 2^-24 with scale 100 * 2^24: 0, 100, 200 and the
    clamp — through the wide source and through the general way."""
    W, H = wh
    L = V.grid(W, H, 1)
    scale = 100.0 * 2.0 ** 24
    rng = np.random.default_rng(7)
    buf = floats.fill_bits(L.samples, "float16")
    wants = []
    for w in L.np_windows(buf):
        w[...] = rng.integers(0, 4, (H, W, 1), dtype=np.uint16)
        wants.append(quant.quantise(w, "float16", scale, 0.0, 255))
    assert sorted(set(np.stack(wants).reshape(-1).tolist())) == [0, 100, 200, 255]
    tf, _ = floats.to_device_floats(ctx.device, buf, "float16")
    out, info = ctx.encode_view_float(L.t_view(tf), scale=scale)
    infos, host = V.infos_of(info), out.cpu().numpy()
    for i, v in enumerate(wants):
        assert host[i, :infos[i].nbytes].tobytes() == orc.encode(v.astype(np.uint8))[0], i


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------

def test_bad_float_sources_are_refused_with_a_text_and_nothing_is_written(ctx):
    import torch

    import dwt_amd

    W, H, n = 72, 68, 4
    FW = 4 * W + 8
    bits = floats.fill_bits((H * 2 + 8) * FW + 64, "float32")
    tf, raw = floats.to_device_floats(ctx.device, bits, "float32")
    stride = int(ctx.lib.dwtx_encode_bound16(W, H, 3))
    out = torch.full((n, stride), 0x5A, dtype=torch.uint8, device=ctx.device)
    info = torch.full((n, C.sizeof(dwt_amd.StreamInfo)), 0x5A, dtype=torch.uint8, device=ctx.device)
    p = tf.data_ptr()
    row = W

    def view(dev=p, sb=4, ch=1, maxval=255, cols=0, pitch=FW, istride=W, bstride=0, cs=0):
        return dwt_amd.View(dev, sb, ch, maxval, cols, pitch, istride, bstride, cs)

    def fmt(type=0, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
        return dwt_amd.FloatFormat(type, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias))

    def encode(v, f, step=0, order=0):
        return ctx.lib.dwtx_encode_view_float(ctx.h, C.byref(v) if v is not None else None, step, order, C.byref(f) if f is not None else None,
                                              W, H, n, 0, out.data_ptr(), stride, info.data_ptr())

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
        "maxval 0": (view(maxval=0), fmt(), {}, b"maxval 0"),
        "maxval negative": (view(maxval=-1), fmt(), {}, b"maxval -1"),
        "maxval beyond 16 bits": (view(maxval=65536), fmt(), {}, b"maxval 65536"),
        # everything dwtx_encode_view_order refuses, with float strides
        "no view": (None, fmt(), {}, b"no view"),
        "channel order": (view(), fmt(), dict(order=2), b"channel order"),
        "row_pitch below a row": (view(pitch=row - 1), fmt(), {}, b"row_pitch"),
        "row_pitch below a stepped row": (view(ch=3, pitch=4 * (W - 1) + 2, istride=4 * W), fmt(), dict(step=4), b"row_pitch"),
        "channels": (view(ch=2), fmt(), {}, b"channels 2"),
        "dev not aligned to the sample": (view(dev=p + 2), fmt(), {}, b"not aligned"),
        "pixel_step below the channels": (view(ch=3, pitch=3 * FW, istride=3 * W), fmt(), dict(step=2), b"pixel_step"),
        "planar with a step": (view(ch=3, cs=H * FW, istride=W), fmt(), dict(step=4), b"planar"),
    }
    for name, (v, f, kw, text) in bad.items():
        assert encode(v, f, **kw) == ERR_ARG, name
        assert text in ctx.lib.dwtx_last_error(), (name, ctx.lib.dwtx_last_error())
    ctx.sync()
    assert (out.cpu().numpy() == 0x5A).all() and (info.cpu().numpy() == 0x5A).all(), "a refused call wrote to dev_out or dev_info"
    assert (floats.bits_of(raw) == bits).all()
    # the bounds themselves are fine: overlapping windows, every maxval a deep picture may have
    good = {"overlapping windows": view(istride=row - 1), "maxval 1": view(maxval=1), "maxval 65535": view(maxval=65535)}
    for name, v in good.items():
        assert encode(v, fmt()) == 0, (name, ctx.lib.dwtx_last_error())
    ctx.sync()
    assert (info.cpu().numpy() != 0x5A).any()


# ---- 8. the encode index ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_the_encode_index_is_that_of_the_same_stream(ctx, kind):
    """set_encode_index under encode_view_float: byte for byte the index the integer encode of the quantised copy leaves."""
    W, H, Cn, maxval, name = 132, 100, 3, 255, "imagenet_inv"
    L = P.nchw(W, H)
    scale, bias = quant.SETS[name](maxval)
    buf = floats.fill_bits(L.samples, kind)
    wants = []
    for i, w in enumerate(L.np_windows(buf)):
        bits, v = quant.window(W, H, Cn, kind, maxval, name, i)
        w[...] = bits
        wants.append(v.astype(np.uint8))
    tf, _ = floats.to_device_floats(ctx.device, buf, kind)
    dev_index = ctx.set_encode_index(L.n, device=True)
    try:
        out, info = ctx.encode_view_float(L.t_view(tf), scale=scale, bias=bias)
        got = EI._rows(ctx, dev_index)
        dout, dinfo = ctx.encode_device(V.to_device(ctx, np.stack(wants)))
        want = EI._rows(ctx, dev_index)
    finally:
        ctx.set_encode_index()
    assert EI._streams_of(ctx, out, info) == [orc.encode(v)[0] for v in wants]
    EI._assert_equal(got, want, f"encode_view_float {kind}")


# ---- 9. the stream contract -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,kind,maxval", [("chw_grid", "float32", 255), ("gray-grid", "float16", V.M16), ("rgb-stack", "bfloat16", 255)])
def test_float_encode_runs_on_the_contexts_stream(layout, kind, maxval):
    """As tests/test_streams_gpu.py has it for the integer encodes: on a context's own non-default stream, with no
    synchronisation, behind a calibrated delay — the source holds a valid decoy until its producer (a copy queued on the
    stream) runs and another right after the call, the outputs are cloned on the stream.  The clones hold the oracle's
    streams of the real pictures: the call waited for its producer and was done before its consumer."""
    import torch

    import test_streams_gpu as TS

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    W, H = 132, 100
    Cn, make = F.LAYOUTS[layout]
    L = make(W, H)
    name = "imagenet_inv"
    scale, bias = quant.SETS[name](maxval)

    def frame(first):
        buf = floats.fill_bits(L.samples, kind)
        for i, w in enumerate(L.np_windows(buf)):
            w[...] = quant.window(W, H, Cn, kind, maxval, name, (first + i) % PICS)[0]
        return torch.from_numpy(buf.view(np.int32 if kind == "float32" else np.int16))

    delay = TS._Delay()
    St = torch.cuda.Stream()
    c = TS._context_on(St)
    try:
        real, decoy, decoy2 = (frame(k).to(c.device) for k in (0, 1, 2))
        src = decoy.clone()
        tv = L.t_view(src.view(floats.torch_dtype(kind)))
        call = lambda out=None, info=None: c.encode_view_float(tv, maxval=maxval, scale=scale, bias=bias, out=out, info=info)
        torch.cuda.synchronize()
        t0, t1 = TS._events(2)
        with torch.cuda.stream(St):
            t0.record()
            out, info = call()   # warm, on the decoy: a join that is lost later leaves the decoy's streams in `out`
            t1.record()
            St.synchronize()
            call_ms = t0.elapsed_time(t1)
            t0.record()
            delay.queue(TS._delay_for(call_ms))
            t1.record()
            src.copy_(real)
            call(out, info)
            src.copy_(decoy2)
            got_out, got_info = out.clone(), info.clone()
        St.synchronize()
        TS._conclusive(f"encode_view_float {layout} {kind}", t0.elapsed_time(t1), call_ms)
        infos, host = V.infos_of(got_info), got_out.cpu().numpy()
        for i in range(L.n):
            want = quant.oracle_encode(W, H, Cn, kind, maxval, name, i % PICS)[0]
            assert infos[i].error == 0 and host[i, :infos[i].nbytes].tobytes() == want, i
    finally:
        c.close()


# ---- 10. round trip ------------------------------------------------------------------------------------------------------------------------

def test_round_trip_through_both_float_calls(ctx):
    """An NCHW float16 batch in [-1, 1]: encode_view_float with (127.5, 127.5), decode_view_float with the inverse pair —
    quant.py's integers through floats.reference, bit for bit."""
    import torch

    W, H, kind = 132, 100, "float16"
    L = P.nchw(W, H)
    buf = floats.fill_bits(L.samples, kind)
    wants = []
    for i, w in enumerate(L.np_windows(buf)):
        bits, v = quant.window(W, H, 3, kind, 255, "unit", i)
        w[...] = bits
        wants.append(v)
    tf, _ = floats.to_device_floats(ctx.device, buf, kind)
    out, info = ctx.encode_view_float(L.t_view(tf), scale=127.5, bias=127.5)
    lens = ctx.stream_lengths(info)
    back_bits = floats.fill_bits(L.samples, kind)
    want = back_bits.copy()
    scale, bias = 1.0 / 127.5, -1.0
    for w, v in zip(L.np_windows(want), wants):
        w[...] = floats.reference(v, kind, scale, bias)
    tb, rawb = floats.to_device_floats(ctx.device, back_bits, kind)
    infos = ctx.decode_view_float(out, lens, L.t_view(tb), scale=scale, bias=bias)
    assert all(I.status == 0 for I in infos)
    assert (floats.bits_of(rawb) == want).all()
