"""CPU: the reference walks of dwtx_decode_view_clips_crop (tests/clipsx.py) held to cases by hand and to clips.decode's full-size
result, the break rule of the float walk, the host's launch arithmetic for float groups (the carry pictures), the expansion of
per-clip origins, and dwtx_view_clips_crop_check with every refusal's text.  Needs no device."""
import inspect

import numpy as np
import pytest

import clips
import clipsx
import deep
import delta
import floats
import levels
import orc
import test_delta_cpu as DC

RANGES = delta.RANGES

# the (n, period, DWTX_OPT_DECODE_PARTS) of the GPU file's carry cases
CARRY_CASES = [(15, 2, 4), (11, 3, 4)]


# ---- by hand -----------------------------------------------------------------------------------------------------------------------

def tiny_stack():
    """Two clips of two 16x12 gray pictures, whole streams: every window decodes to its own frame."""
    W, H, period = 16, 12, 2
    fr = [((np.arange(H * W).reshape(H, W, 1) * (3 + i) + 11 * i) % 256).astype(np.uint8) for i in range(4)]
    return W, H, period, fr, clips.streams(fr, period)


def test_the_integer_walk_by_hand():
    W, H, period, fr, datas = tiny_stack()
    cw, ch, origins = 5, 3, [(2, 1), (11, 9)]   # (clip 1: the far corner)
    initial = [np.full((ch, cw, 1), 77, np.uint8) for _ in fr]
    windows, results = clipsx.decode(datas, initial, period, W, H, 1, 0, 255, cw, ch, origins)
    for i, w in enumerate(windows):
        x0, y0 = origins[i // period]
        assert (w == fr[i][y0:y0 + ch, x0:x0 + cw]).all() and w is results[i], i
    # an unreadable link keeps what lay there, and nothing follows it in a clip of two
    bad = list(datas)
    bad[1] = b"\xff\xff" + bad[1][2:]
    windows, results = clipsx.decode(bad, initial, period, W, H, 1, 0, 255, cw, ch, origins)
    assert results[1] is None and (windows[1] == 77).all() and (windows[2] == fr[2][9:12, 11:16]).all()


def test_the_float_walk_by_hand():
    W, H, period, fr, datas = tiny_stack()
    cw, ch, origins = 5, 3, [(2, 1), (11, 9)]
    written, why = clipsx.decode_float(datas, period, W, H, 1, 0, 255, cw, ch, origins)
    assert why == ["key", "link", "key", "link"]
    for i, v in enumerate(written):
        x0, y0 = origins[i // period]
        assert (v == fr[i][y0:y0 + ch, x0:x0 + cw]).all(), i
    bits = clipsx.float_bits(written, "float32", 0.5, -3.0)
    want = (fr[1][1:4, 2:7].astype(np.float32) * np.float32(0.5) - np.float32(3.0)).view(np.uint32)
    assert (bits[1] == want).all()
    # an unreadable key: its whole clip stays untouched, the next clip does not
    bad = list(datas)
    bad[0] = b"\xff\xff" + bad[0][2:]
    written, why = clipsx.decode_float(bad, period, W, H, 1, 0, 255, cw, ch, origins)
    assert why == ["unreadable key", "dead", "key", "link"] and written[0] is None and written[1] is None and written[3] is not None


# ---- whole streams: the crop of the walk is the walk of the crops ---------------------------------------------------------------------

def whole_rows(W, H, C, lo, hi, n, period):
    """Streams that all reach their finest level, with the cut residuals and the cut key of the clamp fixtures among them: every
    clamp of a key and of a link acts, and the clip goes on from clamped samples."""
    datas = clips.streams(clips.frames(W, H, C, lo, hi, n), period)
    links = [i for i in range(n) if not clips.is_key(i, period)]
    datas[links[1]] = delta.cut_fixture(W, H, C, lo, hi, 0.6)[0]
    datas[(n - 1) // period * period] = clips.cut_key(W, H, C, lo, hi)[0]
    return datas


@pytest.mark.parametrize("rng", RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
def test_both_walks_equal_the_slice_of_the_full_size_walk(C, rng):
    W, H, n, period = 132, 72, 7, 3
    lo, hi = rng
    dt = delta.dtype_of(lo, hi)
    datas = whole_rows(W, H, C, lo, hi, n, period)
    full, results = clips.decode(datas, [np.zeros((H, W, C), dt)] * n, period, W, H, C, lo, hi)
    assert not any(r is None or r is clips.UNTOUCHED for r in results)
    assert (full[2] != clips.frames(W, H, C, lo, hi, n)[2]).any()   # (window 2, the cut link: not its frame, clamps at work)
    cw, ch, origins = 33, 21, [(0, 0), (W - 33, H - 21), (17, 8)]
    at = clipsx.expand(origins, n, period)
    windows, _ = clipsx.decode(datas, [np.zeros((ch, cw, C), dt)] * n, period, W, H, C, lo, hi, cw, ch, origins)
    written, why = clipsx.decode_float(datas, period, W, H, C, lo, hi, cw, ch, origins)
    assert set(why) == {"key", "link"}
    scale, bias = floats.SETS["imagenet"](hi)
    for i in range(n):
        x0, y0 = at[i]
        sl = full[i][y0:y0 + ch, x0:x0 + cw]
        assert (windows[i] == sl).all() and windows[i].dtype == dt, i
        assert (written[i] == sl).all(), i
        for kind in floats.KINDS:
            assert (floats.reference(written[i], kind, scale, bias) == floats.reference(sl, kind, scale, bias)).all()


# ---- the break rule ----------------------------------------------------------------------------------------------------------------

def broken_rows(W, H, C, lo, hi):
    """13 windows, period 4 — clip 0: key, link, link, link (live links behind live links) | clip 1: key cut before its finest
    level, three dead links | clip 2: key, unreadable link, dead, dead | clip 3: key."""
    datas = clips.streams(clips.frames(W, H, C, lo, hi, 13), 4)
    datas[4] = levels.late_prefix(datas[4], W, H, C, orc.geometry(W, H).levels - 2)
    datas[9] = b"\xff\xff" + datas[9][2:]
    return datas


def test_a_break_ends_the_clip():
    W, H, C, lo, hi = 132, 72, 1, 0, 255
    datas = broken_rows(W, H, C, lo, hi)
    more = list(datas)   # clip 0 with a link cut before its finest level behind a live link
    more[2] = levels.late_prefix(more[2], W, H, C, orc.geometry(W, H).levels - 2)
    written, why = clipsx.decode_float(datas, 4, W, H, C, lo, hi, 40, 30, None)
    assert why == ["key", "link", "link", "link", "cut key", "dead", "dead", "dead", "key", "unreadable link", "dead", "dead", "key"]
    written2, why2 = clipsx.decode_float(more, 4, W, H, C, lo, hi, 40, 30, None)
    assert why2[:4] == ["key", "link", "cut link", "dead"]
    seen = set(why) | set(why2)
    assert {"cut key", "unreadable link", "cut link"} <= seen          # each of the three kinds of break occurs
    assert any(a == "link" and b == "link" for a, b in zip(why, why[1:]))   # a live link follows a live link
    assert [v is None for v in written] == [w not in ("key", "link") for w in why]
    # the integer walk goes on where the float walk stops: window 3 of `more` is built on what lay in window 2
    initial = [np.full((30, 40, C), 9, np.uint8) for _ in more]
    _, results = clipsx.decode(more, initial, 4, W, H, C, lo, hi, 40, 30, None)
    assert results[2] is clips.UNTOUCHED and results[3] is not None and results[3] is not clips.UNTOUCHED and written2[3] is None


# ---- the origins ---------------------------------------------------------------------------------------------------------------------

def test_per_clip_origins_are_spelled_out_per_picture():
    import dwt_amd

    assert clipsx.expand(None, 5, 2) == [(0, 0)] * 5
    assert clipsx.expand([(1, 2), (3, 4), (5, 6)], 5, 2) == [(1, 2), (1, 2), (3, 4), (3, 4), (5, 6)]
    assert clipsx.expand([(7, 8)], 5, 9) == [(7, 8)] * 5
    assert clipsx.nclips(11, 4) == 3 and clipsx.nclips(12, 4) == 3 and clipsx.nclips(11, 1) == 11 and clipsx.nclips(3, 50) == 1
    assert dwt_amd.clip_origins(None, 11, 4) is None
    assert dwt_amd.clip_origins((3, 4), 11, 4) == [(3, 4)] * 3
    assert dwt_amd.clip_origins([(1, 2), (3, 4), (5, 6)], 11, 4) == [(1, 2), (3, 4), (5, 6)]
    for bad in ([(1, 2)] * 11, [(1, 2)] * 2, [(1, 2)] * 4):
        with pytest.raises(ValueError, match="origins"):
            dwt_amd.clip_origins(bad, 11, 4)


# ---- the launches of a float call ------------------------------------------------------------------------------------------------------

def check_launches(groups, whole, n, period):
    """launches() against the walk's flags, and the carry pictures' discipline: a launch reads the picture the launch before it
    wrote, never the one it writes itself."""
    L = clipsx.launches(groups, whole, n, period)
    live, flag = [], False
    for i in range(n):
        flag = whole[i] if clips.is_key(i, period) else (flag and whole[i])
        live.append(flag)
    covered = [False] * n
    prev_written = None
    for first, count, reads, writes, slot_read, slot_written in L:
        assert count >= 1 and all(live[first:first + count]) and not any(covered[first:first + count])
        for i in range(first, first + count):
            covered[i] = True
        assert reads == (not clips.is_key(first, period))
        if reads:   # the launch before this one ended at first - 1, mid-clip, and left its running sample
            assert covered[first - 1] and slot_read == prev_written and slot_read is not None
        assert writes == (first + count < n and not clips.is_key(first + count, period))
        if writes:
            assert slot_written in (0, 1) and slot_written != slot_read and slot_written != prev_written
            prev_written = slot_written
    assert covered == live
    return L


def test_dead_first_segments_are_dropped_and_the_carry_alternates():
    # whole streams: every part is one group
    for n, period, K in CARRY_CASES + [(11, 4, 2), (11, 5, 2), (11, 1, 4), (11, 11, 4), (12, 4, 0)]:
        parts = deep.decoder_parts(n, K)
        L = check_launches(clipsx.groups_of(parts, [True] * n), [True] * n, n, period)
        assert [(f, c) for f, c, *_ in L] == [(p[0], len(p)) for p in parts]
    # a group that starts mid-clip on a dead clip starts at its first key; one that holds no key is not launched at all
    n, period = 11, 4
    whole = [True] * n
    whole[1] = False
    groups = clipsx.groups_of(deep.decoder_parts(n, 2), whole)   # [0,5): one window each; [5,11): one group
    assert groups == [(0, 1), (2, 1), (3, 1), (4, 1), (5, 6)]
    L = check_launches(groups, whole, n, period)
    assert [(f, c, r) for f, c, r, *_ in L] == [(0, 1, False), (4, 1, False), (5, 6, True)]
    whole = [True] * n
    whole[4] = False
    L = check_launches(clipsx.groups_of(deep.decoder_parts(n, 2), whole), whole, n, period)
    assert [(f, c, r) for f, c, r, *_ in L] == [(0, 1, False), (1, 1, True), (2, 1, True), (3, 1, True), (8, 3, False)]
    whole = [True] * n
    whole[5] = False
    L = check_launches(clipsx.groups_of(deep.decoder_parts(n, 4), whole), whole, n, period)   # [0,2) [2,5) | [5,8): 6, 7 dead | [8,11)
    assert [(f, c) for f, c, *_ in L] == [(0, 2), (2, 3), (8, 3)]
    # every pattern of whole windows of a small stack, under every period and number of parts
    for n in (4, 7):
        for period in range(1, n + 1):
            for K in (1, 2, 4):
                for bits in range(1 << n):
                    whole = [bool(bits >> i & 1) for i in range(n)]
                    check_launches(clipsx.groups_of(deep.decoder_parts(n, K), whole), whole, n, period)


@pytest.mark.parametrize("case", CARRY_CASES, ids=lambda c: "n%d-period%d-parts%d" % c)
def test_a_group_reads_and_writes_a_carry_in_one_launch(case):
    """The GPU file's carry cases: by the arithmetic of the decoder's parts (deep.decoder_parts, which tests/test_clips_gpu.py's
    "[0,5) [5,11)" rests on) at least one group both starts and ends mid-clip with two segments or more — in (15, 2, 4) with
    three, so that the segment that reads and the one that writes are different workgroups with one between them."""
    n, period, K = case
    parts = deep.decoder_parts(n, K)
    both = [p for p in parts if not clips.is_key(p[0], period) and p[-1] + 1 < n and not clips.is_key(p[-1] + 1, period)
            and len(clips.segments(p[0], len(p), period)) >= 2]
    assert both, parts
    L = clipsx.launches([(p[0], len(p)) for p in parts], [True] * n, n, period)
    assert any(r and w and a != b for _, _, r, w, a, b in L)
    if case == (15, 2, 4):
        assert [list(p) for p in parts][1] == [3, 4, 5, 6] and len(clips.segments(3, 4, 2)) == 3
    # n = 11 with two parts does not give it: [5,11) ends with the stack
    assert not any(r and w for _, _, r, w, _, _ in clipsx.launches([(0, 5), (5, 6)], [True] * 11, 11, 4))


# ---- dwtx_view_clips_crop_check ------------------------------------------------------------------------------------------------------

def test_clips_crop_check_takes_and_refuses():
    import dwt_amd

    W, H, n, cw, ch = 64, 48, 5, 20, 10
    ptr = 1 << 24
    check = dwt_amd.view_clips_crop_check
    f32 = dwt_amd.float_format("float32", (0.5, 0.25, 2.0), (1.0, 2.0, 3.0))
    f16 = dwt_amd.float_format("bfloat16")
    stack = DC._fields(cw, ch, 1, n, cw, cw * ch)
    rgb = DC._fields(cw, ch, 3, n, 3 * cw, 3 * cw * ch)
    for period in (1, 2, n, n + 3):
        k = clipsx.nclips(n, period)
        assert check(stack, ptr, period, (W, H)) == (0, "")
        assert check(stack, ptr, period, (W, H), origins=[(W - cw, H - ch)] * k) == (0, "")
        assert check(stack, ptr, period, (W, H), origins=[(3, 5)] * k, sample_bytes=2, signed=True, minval=-1024, maxval=3071) == (0, "")
        assert check(stack, ptr, period, (W, H), origins=[(3, 5)] * k, sample_bytes=4, fmt=f32) == (0, "")
        assert check(rgb, ptr, period, (W, H), sample_bytes=2, fmt=f16, maxval=4095) == (0, "")
        assert check(rgb, ptr, period, (W, H), sample_bytes=2, fmt=f16, signed=True, minval=-1024, maxval=3071) == (0, "")
    # thin crops, planar and stepped crop-sized windows
    assert check(DC._fields(1, ch, 1, n, 1, ch), ptr, 2, (W, H), origins=[(W - 1, 0)] * 3) == (0, "")
    assert check(DC._fields(cw, 1, 1, n, cw, cw), ptr, 2, (W, H), origins=[(0, H - 1)] * 3) == (0, "")
    assert check(DC._fields(cw, ch, 3, n, cw, 3 * cw * ch, channel_stride=cw * ch), ptr, 3, (W, H)) == (0, "")
    assert check(DC._fields(cw, ch, 3, n, 4 * cw, 4 * cw * ch, pixel_step=4), ptr, 3, (W, H), sample_bytes=4, fmt=f32) == (0, "")
    # a full-size crop is held to the clips check
    full = DC._fields(W, H, 1, n, W, W * H)
    assert check(full, ptr, 2, (W, H)) == dwt_amd.view_clips_check(full, ptr, 2) == (0, "")
    for kw in (dict(sample_bytes=1, signed=True), dict(sample_bytes=2, minval=-5), dict(sample_bytes=1, maxval=100),
               dict(sample_bytes=2, signed=True, minval=100, maxval=50)):
        assert check(full, ptr, 2, (W, H), **kw) == dwt_amd.view_clips_check(full, ptr, 2, **kw) != (0, ""), kw
    over = DC._fields(W, H, 1, n, W, W * H - W)
    assert check(over, ptr, 2, (W, H)) == dwt_amd.view_clips_check(over, ptr, 2) != (0, "")
    assert check(full, ptr, 0, (W, H)) == dwt_amd.view_clips_check(full, ptr, 0) != (0, "")

    def refused(start, *also, **kw):
        args = dict(fields=stack, pointer=ptr, period=2, size=(W, H))
        args.update(kw)
        rc, text = check(**args)
        assert rc == -3 and text.startswith("clips view:") and text.startswith(start) and all(a in text for a in also), text

    # everything the clips call refuses
    refused("clips view: period 0", period=0)
    refused("clips view: no view", fields=None, pointer=0)
    refused("clips view:", "1-byte samples", sample_bytes=1, signed=True)
    refused("clips view:", "without sgn", sample_bytes=2, minval=-5)
    refused("clips view:", "minval < maxval", sample_bytes=2, signed=True, minval=100, maxval=50)
    refused("clips view: maxval 100", maxval=100)
    refused("clips view:", pointer=0)
    refused("clips view: row_pitch", fields=DC._fields(cw, ch, 1, n, cw - 1, cw * ch))
    refused("clips view: windows overlap", fields=DC._fields(cw, ch, 1, n, cw, cw * ch - cw))
    refused("clips view:", "channels 2", fields=DC._fields(cw, ch, 2, n, 2 * cw, 2 * cw * ch))
    refused("clips view: pixel_step", fields=DC._fields(cw, ch, 3, n, 2 * cw, 3 * cw * ch, pixel_step=2))
    refused("clips view: unsupported image size 4x4", size=(4, 4))
    # the crop and its origins
    refused("clips view: crop 65x10", fields=DC._fields(W + 1, ch, 1, n, W + 1, (W + 1) * ch))
    refused("clips view: crop 20x49", fields=DC._fields(cw, H + 1, 1, n, cw, cw * (H + 1)))
    refused("clips view: origin (45, 0) of clip 1", origins=[(0, 0), (W - cw + 1, 0), (0, 0)])
    refused("clips view: origin (0, 39) of clip 2", origins=[(0, 0), (0, 0), (0, H - ch + 1)])
    refused("clips view: origin (-1, 0) of clip 0", origins=[(-1, 0), (0, 0), (0, 0)])
    # the float format
    bad = dwt_amd.float_format("float32")
    bad.type = 3
    refused("clips view: float type 3", sample_bytes=4, fmt=bad)
    refused("clips view: sample_bytes 2 does not match the float type", sample_bytes=2, fmt=f32)
    refused("clips view: sample_bytes 4 does not match the float type", sample_bytes=4, fmt=f16)
    for field, c, v in (("scale", 1, float("inf")), ("bias", 2, float("nan")), ("scale", 0, float("nan"))):
        bad = dwt_amd.float_format("float32")
        getattr(bad, field)[c] = v
        refused("clips view: scale[%d]" % c, "finite", sample_bytes=4, fmt=bad)
    refused("clips view:", "without sgn", sample_bytes=4, fmt=f32, minval=-5)
    # the period is looked at before the crop, the crop before the format, the format before the view
    refused("clips view: period -1", period=-1, fields=DC._fields(W + 1, ch, 1, n, W + 1, (W + 1) * ch))
    bad = dwt_amd.float_format("float32")
    bad.type = 7
    refused("clips view: crop 65x10", fields=DC._fields(W + 1, ch, 1, n, W + 1, (W + 1) * ch), sample_bytes=4, fmt=bad)
    refused("clips view: float type 7", fields=DC._fields(cw, ch, 1, n, cw - 1, cw * ch), sample_bytes=4, fmt=bad)


# ---- the ABI and the Python surface -------------------------------------------------------------------------------------------------

def test_the_entry_points_are_declared_typed_and_exported():
    from dwt_amd import _lib
    import dwt_amd
    import test_abi

    lib = _lib.load()
    declared = test_abi.declared_symbols()
    for name in ("dwtx_decode_view_clips_crop", "dwtx_view_clips_crop_check"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    params = inspect.signature(dwt_amd.Context.decode_view_clips_crop).parameters
    assert list(params)[:7] == ["self", "streams", "lens", "into", "period", "size", "origins"]
    assert {"maxval", "scale", "bias", "stepped", "order", "signed", "minval"} <= set(params)
    assert not {"flip", "levels_max", "key", "windows"} & set(params)
    # decode_view_clips itself is not touched
    assert not {"size", "origins", "scale", "bias"} & set(inspect.signature(dwt_amd.Context.decode_view_clips).parameters)
