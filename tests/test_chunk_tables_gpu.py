"""GPU: the decoder's chunk tables (unpack.hip: k_link_first / k_link_work leave one 64-bit record per 128-bit chunk in
`cs`; k_scan_reduce, k_scan_parts and k_scan_final turn the records into cs, ct, cg, exitX and breaks in place; DESIGN.md
4.4).  Nothing reads the tables but the token walk and k_hopbits, so every case decodes with ctx.decode_planes and compares
with the oracle's decode of the same bytes: coefficients, status, level, planes and missing; `truncated`, which the oracle
does not report, must be 0 for a whole stream and the same whichever way a stream is decoded.  The streams put the
tables' edges where the kernels change path: chunk counts on, before and after multiples of a scan block (1024 chunks)
and of a quad of chunks, records that do not join their predecessor or are dead, both path families, tables that are
made a second time for a part of the batch, the indexed walk, and streams of one to four chunks."""
import functools

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

W0 = H0 = 512


@functools.lru_cache(maxsize=None)
def _oracle(data, W, H, Cn):
    return orc.decode_stage(data, W, H, Cn, -1)


def check(ctx, streams, W, H, Cn, must_decode=True):
    """Decodes `streams` in one call and compares every image with the oracle (tests/test_count_skip_gpu.py both_ways).
    must_decode: the oracle reads every stream, with at most 16 planes — the documented exception (status 2, DESIGN.md
    section 7) and an unreadable stream (status 1) are then failures, not ways out.  -> [(status, truncated)]"""
    lin, infos = ctx.decode_planes(streams, W, H, Cn)
    lin = lin.cpu().numpy().reshape(len(streams), Cn, W * H)
    for i, data in enumerate(streams):
        ref = _oracle(data, W, H, Cn)
        if must_decode:
            assert ref is not None and max(ref[3]) <= 16, i
        if ref is None:
            assert infos[i].status == 1, i
            continue
        rlin, level, missing, planes = ref
        if max(planes) > 16:
            assert infos[i].status == 2, i
            continue
        assert infos[i].status == 0, i
        assert list(infos[i].planes)[:Cn] == planes, i
        assert infos[i].level == level, i
        assert list(infos[i].missing) == missing.tolist(), i
        assert (lin[i] == rlin).all(), i
    return [(info.status, info.truncated) for info in infos]


def check_alone_and_together(ctx, streams, W, H, Cn, must_decode=True):
    """Each stream in a call of its own (one image: both path families) and all in one call (one family, per-image chunk
    counts, four parts): the same status and `truncated` both ways."""
    alone = [check(ctx, [data], W, H, Cn, must_decode)[0] for data in streams]
    assert check(ctx, streams, W, H, Cn, must_decode) == alone
    return alone


@functools.lru_cache(maxsize=None)
def base_stream():
    """7 829 chunks: 8 scan blocks, 4 workgroup stretches of k_link_first"""
    data, _ = orc.encode(orc.synth(W0, H0, 1, 45, 0))
    assert len(data) == 125263
    return data


EDGES = (1022, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145)


@functools.lru_cache(maxsize=None)
def edge_streams():
    """nch + 1 on, before and after a multiple of 1024 and of 4: the last chunk holds one byte, or all sixteen"""
    data = base_stream()
    return [data[:c] for n in EDGES for c in (16 * n - 15, 16 * n)]


def test_scan_block_edges(ctx, opts):
    streams = edge_streams()
    assert len(streams) == 26
    alone = check_alone_and_together(ctx, streams, W0, H0, 1)
    opts.set("decode_parts", 2)
    assert check(ctx, streams, W0, H0, 1) == alone


def damaged_streams():
    data = base_stream()
    out = []
    rng = np.random.default_rng(5150)
    for third in range(3):
        lo, hi = max(6, third * len(data) // 3), (third + 1) * len(data) // 3
        for _ in range(8):
            b = bytearray(data)
            b[int(rng.integers(lo, hi))] ^= int(rng.integers(1, 256))
            out.append(bytes(b))
    # stretches where no token fits (all ones: dead paths) or every path is one long run of zeros, over a scan block's
    # edge (chunk 1024 begins at byte 16384, chunk 2048 at 32768, chunk 4096 at 65536) and away from one
    for at, count, byte in ((20000, 64, 0xFF), (20000, 64, 0x00), (16376, 48, 0xFF), (32748, 40, 0x00), (60000, 4096, 0x00),
                            (90000, 2048, 0xFF), (32764, 16, 0xAA), (65504, 64, 0x55)):
        b = bytearray(data)
        b[at:at + count] = bytes([byte]) * count
        out.append(bytes(b))
    return out


def test_dead_paths_and_records_that_do_not_join(ctx, opts):
    streams = damaged_streams()
    assert len(streams) == 32
    check_alone_and_together(ctx, streams, W0, H0, 1)


@pytest.mark.parametrize("shape, seed", [((512, 512, 1), 45), ((256, 192, 1), 42), ((96, 64, 3), 43)])
def test_both_families_from_the_start(ctx, opts, shape, seed):
    W, H, Cn = shape
    data, _ = orc.encode(orc.synth(W, H, Cn, seed, 0))
    opts.set("two_families", 1)
    assert check(ctx, [data, data, data], W, H, Cn) == [(0, 0)] * 3


def test_tables_made_twice_for_a_part_of_the_batch(ctx, opts):
    """tests/test_pack_gpu.py's parity-locked rings give the one-family walk up: those images get fresh tables with both
    families (k_part_reset) and are walked again; the others keep the tables they have."""
    import dwt_amd
    from test_pack_gpu import _parity_locked_planes

    data = base_stream()
    locked = [orc.encode_lin(_parity_locked_planes(W0, H0, sign, 0), W0, H0)[0] for sign in (1, -1)]
    batch = [data, data[:16 * 2048 - 15], data, locked[0], data[:16 * 4097], data, locked[1], data[:16 * 6144]]
    got = check(ctx, batch, W0, H0, 1)
    assert all(got[i] == (0, 0) for i in (0, 2, 3, 5, 6))
    opts.set("no_second_walk", 1)
    with pytest.raises(dwt_amd.DwtxError):   # (the locked ones really do give up)
        ctx.decode_planes(batch, W0, H0, 1)


def test_sidecar_index(ctx, opts):
    """An index made by an earlier decode of the same streams: only a stream that was decoded to its end gets one, so the
    whole stream (twice: a part of its own, walked one wave per segment) stands beside a part of two cuts that is
    walked serially.  Then a foreign index (another picture's) for all four, which is turned down: the serial walk starts
    over on the tables that are there."""
    import dwt_amd

    data = base_stream()
    streams = [data, data, data[:16 * 2049 - 15], data[:16 * 6143]]
    other, _ = orc.encode(orc.synth(W0, H0, 1, 46, 0))
    n = len(streams)
    try:
        foreign = ctx.set_index(None, n)
        check(ctx, [other] * n, W0, H0, 1)
        made = ctx.set_index(None, n)
        plain = check(ctx, streams, W0, H0, 1)
        assert all(ix[i].magic == dwt_amd.INDEX_MAGIC for ix in (made, foreign) for i in range(n))
        assert [made[i].nsegs > 0 for i in range(n)] == [True, True, False, False] and all(foreign[i].nsegs > 0 for i in range(n))
        ctx.set_index(made, 0)
        opts.set("no_index_fallback", 1)   # a rejected index would be an error: the whole streams' are accepted
        assert check(ctx, streams, W0, H0, 1) == plain
        opts.set("no_index_fallback", 0)
        ctx.set_index(foreign, 0)
        assert check(ctx, streams, W0, H0, 1) == plain
        opts.set("no_index_fallback", 1)
        with pytest.raises(dwt_amd.DwtxError):   # (it really is turned down)
            ctx.decode_planes(streams, W0, H0, 1)
    finally:
        ctx.set_index()


def test_one_chunk_short(ctx, opts):
    """nch 1 to 4 (3 after rounding, or 7): no chunk has a predecessor worth the name, and the scan's only block is
    mostly sentinel.  The oracle cannot read the shortest, and shows a truncated picture for the others."""
    W, H, Cn = 128, 128, 1
    data, _ = orc.encode(orc.synth(W, H, Cn, 41, 0))
    got = check_alone_and_together(ctx, [data[:c] for c in (7, 16, 17, 32, 48, 63, 64)], W, H, Cn, must_decode=False)
    assert all(status == 1 or truncated for status, truncated in got)
