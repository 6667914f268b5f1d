"""GPU: the sidecar index written by the ENCODER (dwtx_ctx_set_encode_index, pack.hip k_index) — byte for byte the index
the decoder's serial walk makes of the same stream (header and seg[:nsegs]), so that a fresh stream can be decoded the
fast way at once.  The yardsticks are the decoder-made index (ctx.set_index(None, n) + ctx.decode_planes, which
tests/test_index_gpu.py tests) and the oracle (orc.encode, orc.decode_stage); none of them is the code under test."""
import ctypes

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 1), (53, 37, 3), (255, 257, 1), (360, 640, 3), (512, 512, 1), (1080, 1920, 3)]
SEEDS = (3, 4, 5, 6, 7)
HEAD = 32   # bytes of dwtx_index before seg[]


def _pictures(shape):
    """orc.synth seeds 3..7 of both kinds: one batch of ten."""
    H, W, Cn = shape
    return [orc.synth(W, H, Cn, seed, kind) for kind in (0, 1) for seed in SEEDS]


def _decoder_made(ctx, streams, W, H, Cn):
    """The yardstick: what a plain decode of the streams notes as their indices, with its planes and records."""
    made = ctx.set_index(None, len(streams))
    lin, infos = ctx.decode_planes(streams, W, H, Cn)
    ctx.set_index()
    return made, lin.cpu().numpy(), infos


def _rows(ctx, dev_index):
    import dwt_amd

    ctx.sync()
    return [dwt_amd.index_from_row(r) for r in dev_index.cpu()]


def _streams_of(ctx, out, info):
    lens = ctx.stream_lengths(info).cpu().numpy()
    host = out.cpu().numpy()
    return [host[i, : int(lens[i])].tobytes() for i in range(len(lens))]


def _assert_equal(enc, dec, what=""):
    assert len(enc) == len(dec)
    for i, (e, d) in enumerate(zip(enc, dec)):
        n = d.nsegs
        print(f"{what} image {i}: nsegs enc {e.nsegs} dec {n}, stream_bits enc {e.stream_bits} dec {d.stream_bits}, "
              f"entered inside a run: {sum(1 for k in range(max(n, 0)) if d.seg[k].cnt)}")
        assert e.nsegs == n and n > 0, (what, i)
        eb, db = bytes(e)[: HEAD + 32 * n], bytes(d)[: HEAD + 32 * n]
        if eb != db:
            for k in range(n):
                a, b = e.seg[k], d.seg[k]
                ta, tb_ = [(f, getattr(a, f)) for f, _ in a._fields_], [(f, getattr(b, f)) for f, _ in b._fields_]
                if ta != tb_:
                    print(f"  first difference at segment {k}: enc {ta} dec {tb_}")
                    break
        assert eb == db, (what, i)


_INFO_FIELDS = ("status", "level", "nsegs", "truncated", "pmax", "bits_used", "zeros_left")   # as test_index_gpu._same_info


def _same_info(a, b):
    for f in _INFO_FIELDS:
        assert getattr(a, f) == getattr(b, f), f
    assert list(a.planes) == list(b.planes) and list(a.missing) == list(b.missing)


def _assert_accepted(ctx, opts, streams, enc, W, H, Cn, winfos):
    """A decode that is offered the encoder's indices and may not fall back: planes like the oracle's, records like the plain decode's."""
    import dwt_amd

    arr = (dwt_amd.Index * len(enc))(*enc)
    opts.set("no_index_fallback", 1)
    ctx.set_index(arr, 0)
    try:
        lin, ginfos = ctx.decode_planes(streams, W, H, Cn)
    finally:
        ctx.set_index()
        opts.set("no_index_fallback", 0)
    lin = lin.cpu().numpy()
    for i, s in enumerate(streams):
        ref = orc.decode_stage(s, W, H, Cn, -1)
        assert (lin[i * Cn:(i + 1) * Cn] == ref[0]).all(), i
        _same_info(ginfos[i], winfos[i])


def _encode_device_with_index(ctx, pix_np, capacity=0):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(np.stack(pix_np))).to(ctx.device)
    dev_index = ctx.set_encode_index(len(pix_np), device=True)
    try:
        out, info = ctx.encode_device(t, capacity=capacity)
        enc = _rows(ctx, dev_index)
    finally:
        ctx.set_encode_index()
    return out, info, enc


@pytest.mark.parametrize("shape", SHAPES)
def test_encode_device_writes_the_index_the_decoder_makes_and_the_decoder_takes_it(ctx, shape, opts):
    H, W, Cn = shape
    pics = _pictures(shape)
    want = [orc.encode(p)[0] for p in pics]
    out, info, enc = _encode_device_with_index(ctx, pics)
    streams = _streams_of(ctx, out, info)
    assert streams == want
    made, _, winfos = _decoder_made(ctx, streams, W, H, Cn)
    _assert_equal(enc, made, f"encode_device {shape}")
    _assert_accepted(ctx, opts, streams, enc, W, H, Cn, winfos)


@pytest.mark.parametrize("shape", SHAPES)
def test_encode_planes_writes_the_same_index(ctx, shape):
    import torch

    H, W, Cn = shape
    pics = _pictures(shape)
    want = [orc.encode(p)[0] for p in pics]
    lin = np.concatenate([orc.stage_dump(p)[1] for p in pics])
    dev_index = ctx.set_encode_index(len(pics), device=True)
    try:
        streams, _ = ctx.encode_planes(torch.from_numpy(lin).to(ctx.device), W, H, Cn)
        enc = _rows(ctx, dev_index)
    finally:
        ctx.set_encode_index()
    assert streams == want
    made, _, _ = _decoder_made(ctx, streams, W, H, Cn)
    _assert_equal(enc, made, f"encode_planes {shape}")


@pytest.mark.parametrize("shape", SHAPES)
def test_host_encode_in_parts_puts_every_index_with_its_image(ctx, shape, opts):
    """dwtx_encode_images cuts a batch of five into parts of two: image i of the call lands in entry i."""
    H, W, Cn = shape
    pics = [orc.synth(W, H, Cn, seed, seed & 1) for seed in SEEDS]
    want = [orc.encode(p)[0] for p in pics]
    opts.set("part_images", 2)
    enc = ctx.set_encode_index(len(pics))
    try:
        streams, _ = ctx.encode(np.stack(pics))
    finally:
        ctx.set_encode_index()
    assert streams == want
    made, _, _ = _decoder_made(ctx, streams, W, H, Cn)
    _assert_equal(list(enc), made, f"host encode {shape}")


def test_a_batch_large_enough_to_run_as_parts_keeps_entry_i_with_image_i(ctx):
    """dwtx_encode_device runs 128 and more images as four parts on streams of their own: every part writes its own entries."""
    H, W, Cn, n = 40, 72, 3, 130
    pix = ctx.synth_pixels(n, H, W, Cn, seed0=11, kind=0)
    dev_index = ctx.set_encode_index(n, device=True)
    try:
        out, info = ctx.encode_device(pix)
        enc = _rows(ctx, dev_index)
    finally:
        ctx.set_encode_index()
    streams = _streams_of(ctx, out, info)
    for i in (0, 31, 32, 64, 65, 97, 129):
        assert streams[i] == orc.encode(orc.synth(W, H, Cn, 11 + i, 0))[0], i
    made, _, _ = _decoder_made(ctx, streams, W, H, Cn)
    _assert_equal(enc, made, "130 images in parts")


def _sparse_pictures(Cn):
    """tests/test_codec_gpu.py::test_almost_empty_pictures_with_runs_of_millions_of_zeros' four 2048x2048 pictures."""
    W = H = 2048
    rng = np.random.default_rng(2048 + Cn)
    pics = []
    for k in range(4):
        pix = np.full((H, W, Cn), 90 + 20 * k, dtype=np.uint8)
        for _ in range(1 + 3 * k):
            pix[int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(0, Cn))] = int(rng.integers(0, 256))
        pics.append(pix)
    return pics


def _small_sparse_pictures():
    """Their small cousins: 128x128 filled with 110 and four pixels set, one generator for the gray and then the RGB picture."""
    W = H = 128
    rng = np.random.default_rng(5)
    pics = {}
    for Cn in (1, 3):
        pix = np.full((H, W, Cn), 110, dtype=np.uint8)
        for _ in range(4):
            pix[int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(0, Cn))] = int(rng.integers(0, 256))
        pics[Cn] = pix
    return pics


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("size", [2048, 128])
def test_segments_entered_inside_a_zero_run(ctx, size, Cn, opts):
    """Almost empty pictures: most segments begin inside a run that an earlier segment's token opened (rle.h:66-78: the
    counter then holds run - zeros taken + 1, the position is behind that token's code and before its sign)."""
    pics = _sparse_pictures(Cn) if size == 2048 else [_small_sparse_pictures()[Cn]]
    W = H = size
    want = [orc.encode(p)[0] for p in pics]
    made, _, winfos = _decoder_made(ctx, want, W, H, Cn)
    # the inputs hold what this test is about (a condition on the yardstick)
    entries = [made[i].seg[k] for i in range(len(pics)) for k in range(made[i].nsegs)]
    inside = sum(1 for e in entries if e.cnt > 0 and (e.desc >> 8) > 0)
    print(f"{size}x{size}x{Cn}: {inside} of {len(entries)} segments entered inside a run")
    assert inside >= 1 and any(e.cnt == 0 for e in entries)
    out, info, enc = _encode_device_with_index(ctx, pics)
    streams = _streams_of(ctx, out, info)
    assert streams == want
    _assert_equal(enc, made, f"sparse {size} C={Cn}")
    _assert_accepted(ctx, opts, streams, enc, W, H, Cn, winfos)


@pytest.mark.parametrize("shape,option", [((53, 37, 3), "exact_orders"), ((512, 512, 1), "exact_orders"),
                                          ((360, 640, 3), "no_square_tiles"), ((512, 512, 1), "no_fine16")])
def test_both_order_passes_and_both_tile_paths_feed_the_index(ctx, shape, option, opts):
    H, W, Cn = shape
    pics = _pictures(shape)
    want = [orc.encode(p)[0] for p in pics]
    opts.set(option, 1)
    out, info, enc = _encode_device_with_index(ctx, pics)
    if option == "exact_orders":
        import dwt_amd

        raw = info.cpu().numpy()
        assert all(dwt_amd.StreamInfo.from_buffer_copy(raw[i].tobytes()).exact_orders == 1 for i in range(len(pics)))
    streams = _streams_of(ctx, out, info)
    assert streams == want
    made, _, winfos = _decoder_made(ctx, streams, W, H, Cn)
    _assert_equal(enc, made, f"{option} {shape}")
    _assert_accepted(ctx, opts, streams, enc, W, H, Cn, winfos)


def _header_only(e, W, H, Cn):
    import dwt_amd

    assert (e.magic, e.W, e.H, e.C, e.nsegs, e.reserved) == (dwt_amd.INDEX_MAGIC, W, H, Cn, 0, 0)


def test_a_flat_picture_in_a_batch_has_no_index_and_the_others_keep_theirs(ctx):
    H, W, Cn = 96, 80, 3
    pics = [orc.synth(W, H, Cn, seed, 0) for seed in (3, 4)] + [np.full((H, W, Cn), 77, dtype=np.uint8)] + \
        [orc.synth(W, H, Cn, seed, 1) for seed in (5, 6)]
    want = [orc.encode(p)[0] for p in pics]
    out, info, enc = _encode_device_with_index(ctx, pics)
    streams = _streams_of(ctx, out, info)
    assert streams == want
    _header_only(enc[2], W, H, Cn)
    made, _, _ = _decoder_made(ctx, streams, W, H, Cn)
    keep = [0, 1, 3, 4]
    _assert_equal([enc[i] for i in keep], [made[i] for i in keep], "beside a flat picture")


@pytest.mark.parametrize("shape", [(131, 77, 3), (512, 512, 1)])
def test_a_stream_that_capacity_cuts_has_no_index(ctx, shape, opts):
    H, W, Cn = shape
    pix = orc.synth(W, H, Cn, 5, 0)
    whole = orc.encode(pix)[0]
    n = len(whole)
    for cut_off in (0, 1):
        opts.set("no_capacity_cut", cut_off)
        out, info, enc = _encode_device_with_index(ctx, [pix], capacity=n // 2)
        assert _streams_of(ctx, out, info)[0] == whole[: n // 2]
        _header_only(enc[0], W, H, Cn)
    opts.set("no_capacity_cut", 0)
    made, _, _ = _decoder_made(ctx, [whole], W, H, Cn)
    for cap in (n, n + 100):   # (n - 1 is left out on purpose: the decoder may still reach the end there)
        out, info, enc = _encode_device_with_index(ctx, [pix], capacity=cap)
        assert _streams_of(ctx, out, info)[0] == whole
        _assert_equal(enc, made, f"capacity {cap} of {n}")


def test_only_the_header_and_the_segments_of_each_record_are_written(ctx):
    """One guard record before and after the array, everything filled with a pattern: the guards and every seg[nsegs:] tail
    keep it; and once dwtx_ctx_set_encode_index(NULL) has ended it, an encode leaves the old array alone."""
    import torch

    import dwt_amd

    H, W, Cn = 120, 200, 3
    pics = [orc.synth(W, H, Cn, 3, 0), np.full((H, W, Cn), 9, dtype=np.uint8), orc.synth(W, H, Cn, 4, 1)]
    t = torch.from_numpy(np.stack(pics)).to(ctx.device)
    n, size = len(pics), ctypes.sizeof(dwt_amd.Index)
    PAT = 0xA5
    # device array (dwtx_encode_device)
    arr = torch.full((n + 2, size), PAT, dtype=torch.uint8, device=ctx.device)
    rc = ctx.lib.dwtx_ctx_set_encode_index(ctx.h, ctypes.c_void_p(arr[1].data_ptr()))
    assert rc == 0
    try:
        ctx.encode_device(t)
        ctx.sync()
    finally:
        ctx.set_encode_index()
    host = arr.cpu().numpy()
    assert (host[0] == PAT).all() and (host[n + 1] == PAT).all()
    nsegs = []
    for i in range(n):
        e = dwt_amd.index_from_row(host[1 + i].tobytes())
        assert e.magic == dwt_amd.INDEX_MAGIC and 0 <= e.nsegs <= dwt_amd.INDEX_MAX_SEGS
        assert (host[1 + i, HEAD + 32 * e.nsegs:] == PAT).all(), i
        nsegs.append(e.nsegs)
    assert nsegs[0] > 0 and nsegs[1] == 0 and nsegs[2] > 0
    arr.fill_(PAT)
    ctx.encode_device(t)   # ended: nothing more is written there
    ctx.sync()
    assert (arr.cpu().numpy() == PAT).all()
    # host array (dwtx_encode_images)
    harr = (dwt_amd.Index * (n + 2))()
    ctypes.memset(harr, PAT, ctypes.sizeof(harr))
    rc = ctx.lib.dwtx_ctx_set_encode_index(ctx.h, ctypes.c_void_p(ctypes.addressof(harr) + size))
    assert rc == 0
    try:
        ctx.encode(np.stack(pics))
    finally:
        ctx.set_encode_index()
    raw = np.frombuffer(bytes(harr), dtype=np.uint8).reshape(n + 2, size)
    assert (raw[0] == PAT).all() and (raw[n + 1] == PAT).all()
    for i in range(n):
        assert harr[1 + i].nsegs == nsegs[i]
        assert (raw[1 + i, HEAD + 32 * nsegs[i]:] == PAT).all(), i
        assert raw[1 + i, : HEAD + 32 * nsegs[i]].tobytes() == host[1 + i, : HEAD + 32 * nsegs[i]].tobytes()
    ctypes.memset(harr, PAT, ctypes.sizeof(harr))
    ctx.encode(np.stack(pics))
    assert bytes(harr) == bytes([PAT]) * ctypes.sizeof(harr)
