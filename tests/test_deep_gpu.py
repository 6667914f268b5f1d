"""GPU: deep pixels (uint16 samples, maxval up to 65535) through the *16 entry points of include/dwtx.h.

The yardstick is tests/deep.py: the oracle's depth-agnostic stages composed into what the reference's algorithm writes
and reads for wider samples (tests/test_deep_cpu.py pins that composition on the whole-file oracle and on the reference
binary's bytes).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu

GUARD = 4096
ERR_ARG = -3


def _r8(v):
    return (v + 7) // 8 * 8


def _infos(info):
    import dwt_amd

    raw = info.cpu().numpy()
    return [dwt_amd.StreamInfo.from_buffer_copy(raw[i].tobytes()) for i in range(raw.shape[0])]


def _encode_device16(ctx, pics, capacity=0):
    """-> (streams as bytes, StreamInfo records); a refused picture's stream is None."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(np.stack(pics))).to(ctx.device)
    out, info = ctx.encode_device16(t, capacity=capacity)
    infos = _infos(info)
    host = out.cpu().numpy()
    return [None if I.error else host[i, :I.nbytes].tobytes() for i, I in enumerate(infos)], infos


def _check_encode(ctx, pics, capacity=0, host=True):
    """encode16 and encode_device16 of one batch against deep_encode: bytes, planes[], root_bits, total_bits."""
    Cn = pics[0].shape[2]
    want = [deep.deep_encode(p, capacity) for p in pics]
    streams, infos = _encode_device16(ctx, pics, capacity)
    for i, (w, st) in enumerate(want):
        print(f"picture {i}: {pics[i].shape} max {int(pics[i].max())} planes {list(st.planes)[:Cn]} bytes {len(w)}")
        assert infos[i].error == 0, i
        assert list(infos[i].planes)[:Cn] == list(st.planes)[:Cn], i
        assert (infos[i].root_bits, infos[i].total_bits) == (st.root_bits, st.total_bits), i
        assert streams[i] == w, i
    if host:
        hstreams, hstats = ctx.encode16(np.stack(pics), capacity)
        for i, (w, st) in enumerate(want):
            assert hstreams[i] == w, i
            assert list(hstats[i].planes)[:Cn] == list(st.planes)[:Cn], i
            assert (hstats[i].root_bits, hstats[i].total_bits) == (st.root_bits, st.total_bits), i
    return [w for w, _ in want], [st for _, st in want]


def _pictures(W, H, Cn):
    """One batch per geometry: every generator, maxval 1023 to 65535 (full-range noise stays within 16 planes up to
    maxval 16383 for gray and 4095 for colour)."""
    pics = [deep.smooth_noise(W, H, Cn, 1023, 1), deep.smooth_noise(W, H, Cn, 4095, 2), deep.smooth_noise(W, H, Cn, 16383, 3),
            deep.smooth_noise(W, H, Cn, 65535, 4), deep.noise(W, H, Cn, 1023, 5), deep.noise(W, H, Cn, 4095, 6),
            deep.checker(W, H, Cn, 4095), deep.blocks(W, H, Cn, 4095, 7)]
    if Cn == 1:
        pics += [deep.noise(W, H, Cn, 16383, 8), deep.checker(W, H, Cn, 16383), deep.blocks(W, H, Cn, 16383, 9)]
    return pics


# ---- 1. encoding ---------------------------------------------------------------------------------------------------

SHAPES = [(256, 200), (1024, 512), (2048, 1000), (131, 77), (1031, 517), (17, 300), (64, 64)]   # W, H


@pytest.mark.parametrize("general", [0, 1], ids=["fused", "no_pixels16"])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("wh", SHAPES)
def test_encode16_equals_the_composed_oracle(ctx, wh, Cn, general, opts):
    """Both entry points on every shape: 256x200, 1024x512 and 2048x1000 take the finest level straight from the
    16-bit pixels, the others cannot; DWTX_OPT_NO_PIXELS16 sends all of them through widened int32 planes."""
    W, H = wh
    opts.set("no_pixels16", general)
    _check_encode(ctx, _pictures(W, H, Cn))


def test_generated_pictures_need_the_planes_the_cpu_found(ctx):
    """Cross-check of the generators against tests/test_deep_cpu.py::test_generators_plane_counts, on the device."""
    W, H = 256, 200
    _, infos = _encode_device16(ctx, [deep.noise(W, H, 3, 4095, 1), deep.checker(W, H, 3, 4095), deep.blocks(W, H, 3, 4095, 1)])
    assert [list(I.planes) for I in infos] == [[13, 14, 14], [2, 0, 14], [13, 15, 14]]


@pytest.mark.parametrize("case", ["rgb_512x512_4095", "gray_1031x517_8191"])
def test_worst_case_pictures_reach_16_planes(ctx, case, opts):
    """The two pictures of the plane bound whose coefficients lie in [2^15, 2^16): the last plane the coder takes.
    With and without the tiles read straight from the pyramid."""
    if case.startswith("rgb"):
        pic = deep.Gain(512, 512).worst_rgb(4095)
    else:
        pic = deep.Gain(1031, 517).worst_gray(8191)
    for no_sq in (0, 1):
        opts.set("no_square_tiles", no_sq)
        _, stats = _check_encode(ctx, [pic, pic[::-1].copy()])
        assert max(stats[0].planes) == 16
    assert (ctx.decode16(deep.deep_encode(pic)[0], int(pic.max())) == pic).all()


def test_a_large_batch_runs_as_parts(ctx, opts):
    """130 pictures: dwtx_encode_device16 cuts batches of 128 and more into parts on streams of their own; the host
    pair runs in parts of 7."""
    W, H, Cn = 96, 80, 3
    pics = [deep.smooth_noise(W, H, Cn, 4095, s) if s % 3 else deep.blocks(W, H, Cn, 4095, s) for s in range(130)]
    opts.set("part_images", 7)
    want, _ = _check_encode(ctx, pics)
    back = ctx.decode16(want, 4095)
    assert all((b == p).all() for b, p in zip(back, pics))


@pytest.mark.parametrize("Cn", [1, 3])
def test_square_tiles_and_exact_orders_do_not_change_a_stream(ctx, Cn, opts):
    W, H = 256, 256
    pics = _pictures(W, H, Cn)
    for name in ("no_square_tiles", "exact_orders", "one_stream"):
        opts.set(name, 1)
        _check_encode(ctx, pics, host=False)
        opts.set(name, 0)


# ---- 2. CAPACITY ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("wh", [(256, 200), (131, 77)])
def test_capacity_cuts_the_stream_where_the_oracle_does(ctx, wh, Cn, opts):
    W, H = wh
    pics = _pictures(W, H, Cn)
    whole = [deep.deep_encode(p)[0] for p in pics]
    for no_cut in (0, 1):
        opts.set("no_capacity_cut", no_cut)
        for capacity in (5, 100, 1000, 5000, 20000):
            want, _ = _check_encode(ctx, pics, capacity, host=capacity in (100, 5000))
            for w, full in zip(want, whole):
                assert len(w) == min(capacity, len(full)) and full.startswith(w)


# ---- 3. decoding ---------------------------------------------------------------------------------------------------

def _cuts(data, st, seed):
    """At least 24 cut points: 6, 7 and 40 bytes, inside the root image, one byte short, the whole stream, and seeded
    ones anywhere."""
    L = len(data)
    hdr = (st.meta_bits + st.root_bits) // 8
    rng = np.random.default_rng(seed)
    cuts = {6, 7, 40, 6 + (hdr - 6) // 3, 6 + 2 * (hdr - 6) // 3, hdr - 1, hdr + 1, L - 1, L}
    cuts |= set(int(v) for v in rng.integers(hdr, L, 22))
    cuts = sorted(c for c in cuts if 6 <= c <= L)
    assert len(cuts) >= 24
    return cuts


def _decode_device16(ctx, rows, W, H, Cn, maxval, levels_max=-1, pix_stride=None, pix_off=0, expect=0):
    """dwtx_decode_device16 of byte strings into a guarded sample buffer, picture i at sample pix_off + i * pix_stride.
    -> (infos, buffer after, buffer before), both uint16."""
    import torch

    import dwt_amd

    n = len(rows)
    stride = _r8(max(len(r) for r in rows) + 64)
    host = np.zeros((n, stride), dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    if pix_stride is None:
        pix_stride = W * H * Cn
    before = np.random.default_rng(n + pix_off).integers(0, 65536, pix_off + n * pix_stride + GUARD, dtype=np.uint16)
    out = torch.from_numpy(before.copy()).to(ctx.device)
    dev = torch.from_numpy(host).to(ctx.device)
    dl = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()
    rc = ctx.lib.dwtx_decode_device16(ctx.h, dev.data_ptr(), stride, dl.data_ptr(), W, H, Cn, n, levels_max,
                                      out.data_ptr() + 2 * pix_off, pix_stride, maxval, C.cast(infos, C.c_void_p))
    assert rc == expect, (rc, ctx.lib.dwtx_last_error())
    return list(infos), out.cpu().numpy(), before


def _check_decodes(ctx, rows, W, H, Cn, maxval, pixels_max=-1, pix_stride=None, pix_off=0):
    """Every row through decode_device16 and decode16 against deep_decode; nothing outside the pictures is written.
    -> the oracle's pictures (None for an unreadable row)."""
    if pix_stride is None:
        pix_stride = W * H * Cn
    refs = [deep.deep_decode(r, W, H, Cn, maxval, pixels_max) for r in rows]
    infos, after, before = _decode_device16(ctx, rows, W, H, Cn, maxval, deep.levels_max(W, H, pixels_max), pix_stride, pix_off)
    want = before.copy()
    for i, ref in enumerate(refs):
        where = f"row {i}: {len(rows[i])} bytes"
        assert (infos[i].status == 0) == (ref is not None), where
        if ref is None:
            assert infos[i].status == 1, where
            continue
        g = orc.geometry(W, H)
        lo = infos[i].level + 1
        assert (g.heights[lo], g.widths[lo], Cn) == ref.shape, where
        o = pix_off + i * pix_stride
        assert (after[o:o + ref.size] == ref.reshape(-1)).all(), where
        want[o:o + ref.size] = ref.reshape(-1)
    bad = np.nonzero(after != want)[0]
    assert bad.size == 0, f"{bad.size} samples outside the pictures changed, first at {bad[0]}"
    outs = ctx.decode16(rows, maxval, pixels_max)
    for i, (o, ref) in enumerate(zip(outs, refs)):
        assert (o is None) == (ref is None), i
        if ref is not None:
            assert o.dtype == np.uint16 and o.shape == ref.shape and (o == ref).all(), i
    return refs


def _prefix_rows(pic, seed):
    data, st = deep.deep_encode(pic)
    return [data] + [data[:c] for c in _cuts(data, st, seed)]   # the whole stream first: the host call reads row 0's header


PREFIX_PICTURES = {   # name -> (picture, maxval, must some prefix leave [0, maxval] before the clamps?)
    "gray_smooth_1023": (lambda: deep.smooth_noise(256, 200, 1, 1023, 1), 1023, False),
    "gray_noise_16383": (lambda: deep.noise(256, 200, 1, 16383, 2), 16383, False),
    "rgb_smooth_65535": (lambda: deep.smooth_noise(256, 200, 3, 65535, 3), 65535, False),
    "rgb_noise_4095": (lambda: deep.noise(256, 200, 3, 4095, 4), 4095, True),
    "rgb_checker_4095": (lambda: deep.checker(256, 200, 3, 4095), 4095, True),
    "rgb_blocks_4095": (lambda: deep.blocks(256, 200, 3, 4095, 5), 4095, True),
    "rgb_odd_noise_4095": (lambda: deep.noise(131, 77, 3, 4095, 6), 4095, True),
    "gray_thin_4095": (lambda: deep.blocks(17, 300, 1, 4095, 7), 4095, False),
}


@pytest.mark.parametrize("general", [0, 1], ids=["fused", "no_pixels16"])
@pytest.mark.parametrize("name", list(PREFIX_PICTURES))
def test_decode16_of_whole_streams_and_prefixes(ctx, name, general, opts):
    """Whole streams give the pixels back; prefixes equal deep_decode in size and in every sample.  The maxval clamps
    only act on truncated colour streams: for the pictures flagged so, at least one tested prefix must have a sample
    that the arithmetic without clamps puts outside [0, maxval] — otherwise the clamps would go untested."""
    make, maxval, clamps = PREFIX_PICTURES[name]
    pic = make()
    H, W, Cn = pic.shape
    opts.set("no_pixels16", general)
    rows = _prefix_rows(pic, seed=len(name))
    refs = _check_decodes(ctx, rows, W, H, Cn, maxval)
    assert (refs[0] == pic).all()
    assert [r is None for r in refs[1:4]] == [True, True, True]   # 6, 7 and 40 bytes: no root image, no plane counts
    if clamps:
        outside = 0
        for r in rows[1:]:
            raw = deep.deep_decode(r, W, H, Cn, maxval, clamp=False)
            outside += raw is not None and bool(((raw < 0) | (raw > maxval)).any())
        print(f"{name}: {outside} of {len(rows) - 1} prefixes leave [0, {maxval}] before the clamps")
        assert outside >= 1


@pytest.mark.parametrize("pixels_max", [0, 300, 5000, 20000])
@pytest.mark.parametrize("name", ["rgb_noise_4095", "gray_noise_16383"])
def test_pixels_cap(ctx, name, pixels_max):
    make, maxval, _ = PREFIX_PICTURES[name]
    pic = make()
    H, W, Cn = pic.shape
    _check_decodes(ctx, _prefix_rows(pic, seed=pixels_max), W, H, Cn, maxval, pixels_max=pixels_max)


def test_decoder_variants(ctx, opts):
    make, maxval, _ = PREFIX_PICTURES["rgb_blocks_4095"]
    pic = make()
    H, W, Cn = pic.shape
    rows = _prefix_rows(pic, seed=1)
    for name, value in (("no_square_tiles", 1), ("decode_parts", 3), ("one_stream", 1), ("two_families", 1)):
        opts.set(name, value)
        _check_decodes(ctx, rows, W, H, Cn, maxval)
        opts.set(name, 0)


# ---- 4. maxval 255: the deep path restates the shipped one ---------------------------------------------------------

@pytest.mark.parametrize("shape", [(200, 256, 3), (77, 131, 3), (200, 256, 1), (64, 64, 3)])
def test_maxval_255_equals_the_8_bit_entry_points(ctx, shape):
    H, W, Cn = shape
    pics = np.stack([orc.synth(W, H, Cn, 21, 0), orc.synth(W, H, Cn, 22, 1)])
    s8, st8 = ctx.encode(pics)
    s16, st16 = ctx.encode16(pics.astype(np.uint16))
    assert s16 == s8 and s8 == [orc.encode(p)[0] for p in pics]
    for a, b in zip(st8, st16):
        assert (a.root_bits, a.total_bits, list(a.planes)) == (b.root_bits, b.total_bits, list(b.planes))
    for k, data in enumerate(s8):
        _, st = deep.deep_encode(pics[k])
        rows = [data] + [data[:c] for c in _cuts(data, st, k)]
        got16 = ctx.decode16(rows, 255)
        got8 = ctx.decode(rows)
        for a, b in zip(got16, got8):
            assert (a is None) == (b is None)
            if a is not None:
                assert a.dtype == np.uint16 and a.shape == b.shape and (a == b).all()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------

def test_a_picture_with_more_than_16_planes_is_refused_alone(ctx):
    W, H, Cn = 256, 200, 3
    pics = [deep.smooth_noise(W, H, Cn, 65535, 1), deep.noise(W, H, Cn, 65535, 2), deep.blocks(W, H, Cn, 4095, 3)]
    assert max(deep.deep_encode(pics[1])[1].planes) > 16
    streams, infos = _encode_device16(ctx, pics)
    assert [I.error for I in infos] == [0, 1, 0]
    assert streams[0] == deep.deep_encode(pics[0])[0] and streams[2] == deep.deep_encode(pics[2])[0]
    arr = np.stack(pics)
    out = np.empty((3, ctx.lib.dwtx_encode_bound16(W, H, Cn)), dtype=np.uint8)
    lens = (C.c_size_t * 3)()
    rc = ctx.lib.dwtx_encode_images16(ctx.h, arr.ctypes.data, W, H, Cn, 3, 0, out.ctypes.data, out.shape[1], C.cast(lens, C.c_void_p), None)
    assert rc == ERR_ARG
    assert ctx.lib.dwtx_last_error() == b"image 1 needs more than 16 bit planes"
    gray = deep.noise(W, H, 1, 65535, 4)
    assert list(deep.deep_encode(gray)[1].planes)[0] == 17
    assert _encode_device16(ctx, [gray])[1][0].error == 1


def test_encode_planes_refuses_planes_alone_in_a_batch(ctx):
    """The stage call on linearised planes of more than 16 bit planes between two good pictures: error = 1 for it, and
    the neighbours' streams are the oracle's (a refused image must not touch the tables of the next one)."""
    import torch

    import dwt_amd

    W, H, Cn = 128, 96, 3
    pics = [deep.smooth_noise(W, H, Cn, 65535, 1), deep.noise(W, H, Cn, 65535, 2), deep.blocks(W, H, Cn, 4095, 3)]
    lins = [orc.linearize(orc.forward(deep.rgb2ycocg(p))) for p in pics]
    assert max(orc.encode_lin(lins[1], W, H)[1].planes) > 16
    lin = torch.from_numpy(np.concatenate(lins)).to(ctx.device)
    stride = ctx.lib.dwtx_encode_bound16(W, H, Cn)
    out = torch.zeros((3, stride), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros((3, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
    assert ctx.lib.dwtx_encode_planes(ctx.h, lin.data_ptr(), W, H, Cn, 3, 0, out.data_ptr(), stride, info.data_ptr()) == 0
    infos = _infos(info)
    assert [I.error for I in infos] == [0, 1, 0]
    host = out.cpu().numpy()
    for i in (0, 2):
        assert host[i, :infos[i].nbytes].tobytes() == orc.encode_lin(lins[i], W, H)[0], i


def test_a_stream_that_claims_more_than_16_planes_is_status_2(ctx):
    W, H, Cn = 96, 64, 3
    rows = [deep.deep_encode(deep.smooth_noise(W, H, Cn, 4095, 1))[0], orc.many_plane_stream(W, H, Cn, [17, 3, 3])]
    infos, _, _ = _decode_device16(ctx, rows, W, H, Cn, 4095)
    assert [I.status for I in infos] == [0, 2]
    import torch

    host = np.zeros((2, _r8(max(len(r) for r in rows) + 64)), dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=ctx.device)
    _, infos8 = ctx.decode_device(torch.from_numpy(host).to(ctx.device), lens, W, H, Cn)
    assert [I.status for I in infos8] == [0, 2]


@pytest.mark.parametrize("maxval", [0, -1, 65536, 1 << 20])
def test_maxval_outside_1_to_65535_is_refused(ctx, maxval):
    import torch

    W, H, Cn = 64, 48, 1
    pic = deep.smooth_noise(W, H, Cn, 1023, 1)
    data = deep.deep_encode(pic)[0]
    _decode_device16(ctx, [data], W, H, Cn, maxval, expect=ERR_ARG)
    with pytest.raises(Exception) as e:
        ctx.decode16(data, maxval)
    assert e.value.rc == ERR_ARG
    planes = torch.zeros((1, H, W), dtype=torch.int32, device=ctx.device)
    out = torch.from_numpy(np.zeros((1, H, W, 1), dtype=np.uint16)).to(ctx.device)
    assert ctx.lib.dwtx_pixels16_from_planes(ctx.h, out.data_ptr(), planes.data_ptr(), W, H, Cn, 1, maxval) == ERR_ARG
    assert ctx.lib.dwtx_transformation_inv_pixels16(ctx.h, out.data_ptr(), planes.data_ptr(), W, H, Cn, 1, maxval) == ERR_ARG


def test_maxval_1_and_65535_are_taken(ctx):
    W, H = 64, 48
    bits = deep.blocks(W, H, 3, 1, 1)
    data = deep.deep_encode(bits)[0]
    assert ctx.encode16(bits)[0] == data and (ctx.decode16(data, 1) == bits).all()
    _check_decodes(ctx, [data, data[:len(data) // 2], data[:len(data) // 4]], W, H, 3, 1)
    _check_decodes(ctx, _prefix_rows(deep.smooth_noise(W, H, 3, 65535, 2), 3), W, H, 3, 65535)


def test_sides_above_32768_are_refused(ctx):
    import torch

    pix = torch.from_numpy(np.zeros(40000 * 8, dtype=np.uint16)).to(ctx.device)
    out = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.device)
    info = torch.zeros(256, dtype=torch.uint8, device=ctx.device)
    for W, H in ((32769, 8), (8, 40000)):
        assert ctx.lib.dwtx_encode_device16(ctx.h, pix.data_ptr(), W, H, 1, 1, 0, out.data_ptr(), 1 << 16, info.data_ptr()) == ERR_ARG
        hp = np.zeros(W * H, dtype=np.uint16)
        ho = np.zeros(1 << 16, dtype=np.uint8)
        lens = (C.c_size_t * 1)()
        assert ctx.lib.dwtx_encode_images16(ctx.h, hp.ctypes.data, W, H, 1, 1, 0, ho.ctypes.data, 1 << 16, C.cast(lens, C.c_void_p), None) == ERR_ARG
        hdr = b"W5" + bytes([(W - 1) & 255, (W - 1) >> 8, (H - 1) & 255, (H - 1) >> 8]) + bytes(100)
        with pytest.raises(Exception) as e:
            ctx.decode16(hdr, 4095)
        assert e.value.rc == ERR_ARG


# ---- 6. the transforms on their own --------------------------------------------------------------------------------

EDGES = [(200, 4), (333, 8), (131, 12), (65, 256), (66, 260), (67, 516), (257, 1028), (1030, 68), (2050, 72), (3, 128), (2, 512)]
TRANSFORM_SHAPES = [(H, W) for H, W in EDGES if H >= 8 and W >= 8] + [(200, 256), (512, 1024), (77, 131), (517, 1031), (300, 17), (64, 64)]


@pytest.mark.parametrize("general", [0, 1], ids=["fused", "no_pixels16"])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("shape", TRANSFORM_SHAPES)
def test_transformation_pixels16_against_the_oracle(ctx, shape, Cn, general, opts):
    """transformation_fwd_pixels16 vs YCoCg-R + orc.forward; planes_from_pixels16 / pixels16_from_planes; and
    transformation_inv_pixels16 of arbitrary pyramids, whose samples the clamps at maxval cut, vs orc.inverse + numpy.
    With DWTX_OPT_NO_PIXELS16 off (shapes with W % 4 == 0 above 64 pixels: the finest level from / to the pixels, the
    edge shapes of the wide kernels among them) and on."""
    import torch

    H, W = shape
    opts.set("no_pixels16", general)
    rng = np.random.default_rng(H * 3 + W + Cn)
    pics = np.stack([deep.noise(W, H, Cn, 65535, 1), deep.smooth_noise(W, H, Cn, 4095, 2), deep.blocks(W, H, Cn, 65535, 3)])
    n = len(pics)
    planar = np.stack([(deep.rgb2ycocg(p) if Cn == 3 else p.astype(np.int32)) for p in pics])   # [n, H, W, C]
    dev = torch.from_numpy(pics).to(ctx.device)
    got = ctx.planes_from_pixels16(dev).cpu().numpy().reshape(n, Cn, H, W)
    assert (got == planar.transpose(0, 3, 1, 2)).all()
    want = np.stack([orc.forward(a) for a in planar]).transpose(0, 3, 1, 2)
    pyr = ctx.transformation_fwd_pixels16(dev)
    assert (pyr.cpu().numpy().reshape(n, Cn, H, W) == want).all()
    for M in (4095, 65535):
        back = ctx.transformation_inv_pixels16(pyr, Cn, M).cpu().numpy()
        ref = np.stack([deep.ycocg2rgb(a, M) if Cn == 3 else np.clip(a, 0, M) for a in planar])
        assert back.dtype == np.uint16 and (back == ref).all(), M
    arb = rng.integers(-9000, 9000, size=(n, H, W, Cn), dtype=np.int32)
    for M in (1, 1023, 4095):
        inv = np.stack([orc.inverse(a) for a in arb])
        ref = np.stack([deep.ycocg2rgb(a, M) if Cn == 3 else np.clip(a, 0, M) for a in inv])
        planes = torch.from_numpy(np.ascontiguousarray(arb.transpose(0, 3, 1, 2)).reshape(n * Cn, H, W)).to(ctx.device)
        assert (ctx.transformation_inv_pixels16(planes, Cn, M).cpu().numpy() == ref).all(), M
        flat = torch.from_numpy(np.ascontiguousarray(inv.transpose(0, 3, 1, 2)).reshape(n * Cn, H, W)).to(ctx.device)
        assert (ctx.pixels16_from_planes(flat, Cn, M).cpu().numpy() == ref).all(), M


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("wh", [(256, 200), (1024, 512), (68, 1030), (260, 66), (72, 2050)])
def test_no_pixels16_on_and_off_give_identical_results(ctx, wh, Cn, opts):
    """DWTX_OPT_NO_PIXELS16 chooses between two paths that must agree: identical streams, identical pixels (whole
    and cut streams), identical pyramids, identical inverses of arbitrary pyramids — compared with each other."""
    import torch

    W, H = wh
    pics = np.stack(_pictures(W, H, Cn))
    dev = torch.from_numpy(pics).to(ctx.device)
    rng = np.random.default_rng(W + H)
    arb = torch.from_numpy(rng.integers(-70000, 70000, size=(len(pics) * Cn, H, W), dtype=np.int32)).to(ctx.device)
    got = []
    for general in (0, 1):
        opts.set("no_pixels16", general)
        streams, infos = _encode_device16(ctx, list(pics))
        cut = [s[:len(s) // 3] for s in streams]
        res = {"streams": streams, "total_bits": [I.total_bits for I in infos],
               "pixels": [ctx.decode16(streams, 65535), ctx.decode16(streams[:1] + cut, 4095)],
               "pyr": ctx.transformation_fwd_pixels16(dev).cpu().numpy(),
               "inv": [ctx.transformation_inv_pixels16(arb, Cn, M).cpu().numpy() for M in (1023, 65535)]}
        got.append(res)
    a, b = got
    assert a["streams"] == b["streams"] and a["total_bits"] == b["total_bits"]
    for x, y in zip(a["pixels"], b["pixels"]):
        assert all((p is None) == (q is None) and (p is None or (p.shape == q.shape and (p == q).all())) for p, q in zip(x, y))
    assert all((p == q).all() for p, q in zip(a["pixels"][0], pics))
    assert (a["pyr"] == b["pyr"]).all()
    assert all((p == q).all() for p, q in zip(a["inv"], b["inv"]))


# ---- 7. buffer bounds ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(128, 128, 1), (72, 100, 3)])
def test_pictures_into_padded_pixel_slots(ctx, shape):
    """pix_stride (in samples) larger than the picture, and pictures an odd number of samples into the buffer: the
    padding and the guard keep their sentinels (checked sample by sample in _check_decodes), for whole, uniformly
    truncated and mixed batches."""
    H, W, Cn = shape
    M = 4095
    fulls = [deep.deep_encode(deep.noise(W, H, Cn, M, s) if s & 1 else deep.smooth_noise(W, H, Cn, M, s))[0] for s in range(4)]
    size = W * H * Cn
    batches = {
        "whole": fulls,
        "uniform": [fulls[0][:len(fulls[0]) // 3]] * 4,
        "mixed": [fulls[0], fulls[1][:len(fulls[1]) // 2], fulls[2][:len(fulls[2]) // 9], fulls[3][:200]],
    }
    for what, rows in batches.items():
        for pad, off in ((0, 0), (1, 0), (4, 0), (16, 0), (4096, 0), (0, 1), (3, 3)):
            infos, after, before = _decode_device16(ctx, rows, W, H, Cn, M, pix_stride=size + pad, pix_off=off)
            hbefore = np.random.default_rng(pad).integers(0, 65536, off + 4 * (size + pad) + GUARD, dtype=np.uint16)
            hafter = hbefore.copy()
            want, hwant = before.copy(), hbefore.copy()
            for i, r in enumerate(rows):
                ref = deep.deep_decode(r, W, H, Cn, M)
                assert (infos[i].status == 0) == (ref is not None), (what, i)
                if ref is None:   # (200 bytes do not hold the colour picture's root image: nothing is written)
                    continue
                o = off + i * (size + pad)
                want[o:o + ref.size] = hwant[o:o + ref.size] = ref.reshape(-1)
            assert (after == want).all(), (what, pad, off)
            stride = _r8(max(len(r) for r in rows) + 64)
            host = np.zeros((4, stride), dtype=np.uint8)
            for i, r in enumerate(rows):
                host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
            lens = (C.c_size_t * 4)(*[len(r) for r in rows])
            ow, oh, oc = (C.c_int * 4)(), (C.c_int * 4)(), (C.c_int * 4)()
            rc = ctx.lib.dwtx_decode_images16(ctx.h, host.ctypes.data, stride, C.cast(lens, C.c_void_p), 4, -1,
                                              hafter.ctypes.data + 2 * off, size + pad, M, ow, oh, oc, None)
            assert rc == 0, ctx.lib.dwtx_last_error()
            assert (hafter == hwant).all(), (what, pad, off)


@pytest.mark.parametrize("shape", [(128, 128, 1), (72, 100, 3)])
def test_a_pixel_stride_below_the_picture_is_refused(ctx, shape):
    H, W, Cn = shape
    rows = [deep.deep_encode(deep.smooth_noise(W, H, Cn, 4095, s))[0] for s in range(3)]
    for ps in (W * H * Cn - 1, W * H * Cn // 2):
        _, after, before = _decode_device16(ctx, rows, W, H, Cn, 4095, pix_stride=ps, expect=ERR_ARG)
        assert (after == before).all()
        stride = _r8(max(len(r) for r in rows) + 64)
        host = np.zeros((3, stride), dtype=np.uint8)
        for i, r in enumerate(rows):
            host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        hbefore = np.random.default_rng(ps).integers(0, 65536, 3 * ps + GUARD, dtype=np.uint16)
        hafter = hbefore.copy()
        lens = (C.c_size_t * 3)(*[len(r) for r in rows])
        ow, oh, oc = (C.c_int * 3)(), (C.c_int * 3)(), (C.c_int * 3)()
        rc = ctx.lib.dwtx_decode_images16(ctx.h, host.ctypes.data, stride, C.cast(lens, C.c_void_p), 3, -1,
                                          hafter.ctypes.data, ps, 4095, ow, oh, oc, None)
        assert rc == ERR_ARG and (hafter == hbefore).all()


def test_encode16_into_a_stride_shorter_than_the_stream(ctx):
    """As the 8-bit calls: slot i holds the stream up to the stride, nothing past a slot changes, nbytes is the whole
    stream's."""
    import torch

    import dwt_amd

    W, H, Cn = 128, 96, 3
    pics = [deep.noise(W, H, Cn, 4095, s) for s in range(3)]
    want = [deep.deep_encode(p)[0] for p in pics]
    dpix = torch.from_numpy(np.stack(pics)).to(ctx.device)
    L = min(len(w) for w in want)
    for stride in (8, _r8(L // 2), _r8(L) - 8):
        before = np.random.default_rng(stride).integers(0, 256, 3 * stride + GUARD, dtype=np.uint8)
        out = torch.from_numpy(before.copy()).to(ctx.device)
        info = torch.zeros((3, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
        assert ctx.lib.dwtx_encode_device16(ctx.h, dpix.data_ptr(), W, H, Cn, 3, 0, out.data_ptr(), stride, info.data_ptr()) == 0
        infos = _infos(info)
        got = out.cpu().numpy()
        for i in range(3):
            assert infos[i].nbytes == len(want[i])
            assert got[i * stride:(i + 1) * stride].tobytes() == want[i][:stride]
        assert (got[3 * stride:] == before[3 * stride:]).all()


# ---- 8. the sidecar index ------------------------------------------------------------------------------------------

HEAD = 32   # bytes of dwtx_index before seg[]


@pytest.mark.parametrize("case", ["rgb_worst_512", "rgb_256x200", "gray_1031x517"])
def test_the_encoders_index_of_a_deep_stream(ctx, case, opts):
    """set_encode_index on a deep encode: the index equals the one a decode of the same stream hands out, and a decode
    that is offered it (and may not fall back) gives the same pixels."""
    import torch

    import dwt_amd

    if case == "rgb_worst_512":
        g = deep.Gain(512, 512)
        pics, M = [g.worst_rgb(4095), deep.noise(512, 512, 3, 4095, 1)], 4095
    elif case == "rgb_256x200":
        pics, M = [deep.blocks(256, 200, 3, 4095, 2), deep.smooth_noise(256, 200, 3, 4095, 3)], 4095
    else:
        pics, M = [deep.smooth_noise(1031, 517, 1, 65535, 4), deep.noise(1031, 517, 1, 16383, 5)], 65535
    H, W, Cn = pics[0].shape
    n = len(pics)
    t = torch.from_numpy(np.stack(pics)).to(ctx.device)
    dev_index = ctx.set_encode_index(n, device=True)
    try:
        out, info = ctx.encode_device16(t)
        ctx.sync()
        enc = [dwt_amd.index_from_row(r) for r in dev_index.cpu()]
    finally:
        ctx.set_encode_index()
    infos = _infos(info)
    host = out.cpu().numpy()
    streams = [host[i, :I.nbytes].tobytes() for i, I in enumerate(infos)]
    assert streams == [deep.deep_encode(p)[0] for p in pics]
    made = ctx.set_index(None, n)
    try:
        plain = ctx.decode16(streams, M)
    finally:
        ctx.set_index()
    for i in range(n):
        k = made[i].nsegs
        print(f"{case} image {i}: {k} segments")
        assert enc[i].nsegs == k and 0 < k <= dwt_amd.INDEX_MAX_SEGS
        assert bytes(enc[i])[:HEAD + 32 * k] == bytes(made[i])[:HEAD + 32 * k], i
    arr = (dwt_amd.Index * n)(*enc)
    opts.set("no_index_fallback", 1)
    ctx.set_index(arr, 0)
    try:
        fast = ctx.decode16(streams, M)
    finally:
        ctx.set_index()
    for p, a, b in zip(pics, plain, fast):
        assert (a == p).all() and (b == p).all()
    # the host pair hands the same indices out
    hix = ctx.set_encode_index(n)
    try:
        hstreams, _ = ctx.encode16(np.stack(pics))
    finally:
        ctx.set_encode_index()
    assert hstreams == streams
    for i in range(n):
        k = made[i].nsegs
        assert bytes(hix[i])[:HEAD + 32 * k] == bytes(made[i])[:HEAD + 32 * k], i
