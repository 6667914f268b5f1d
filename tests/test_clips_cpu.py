"""CPU: clip stacks on the oracle (tests/clips.py) — the fold by hand on a two-clip case, exact round trips of a stack of three
clips, the segments a group of windows falls into against the decode kernel's arithmetic, the conditions the cut key of
tests/test_clips_gpu.py's clamp fixture must meet, dwtx_view_clips_check's refusals with their texts, and the three entry points
declared, typed and exported."""
import inspect

import numpy as np
import pytest

import clips
import deep
import delta
import orc
import signed
import test_delta_cpu as DC

RANGES = [(0, 255)] + signed.RANGES


# ---- the fold --------------------------------------------------------------------------------------------------------------------

def test_the_fold_by_hand_on_two_clips():
    """n = 5, period 3: windows 0 and 3 are keys, decoded alone; 1, 2 and 4 are links onto the window before AS IT LIES THERE.  An
    unreadable key and a key cut before its finest level keep what the caller left — nothing of a coarse picture is written —
    and the links behind them add their residuals to that."""
    import levels

    W, H, C, lo, hi = 132, 72, 1, 0, 255
    fr = clips.frames(W, H, C, lo, hi, 5)
    datas = clips.streams(fr, 3)
    assert datas[0] == deep.deep_encode(fr[0])[0] and datas[3] == deep.deep_encode(fr[3])[0]
    assert datas[1] == delta.stream(fr[1], fr[0])[0] and datas[4] == delta.stream(fr[4], fr[3])[0]
    left = [np.full_like(fr[0], 30 + 40 * i) for i in range(5)]
    # whole streams: the stack comes back, whatever lay there
    windows, results = clips.decode(datas, left, 3, W, H, C, lo, hi)
    assert all((w == f).all() for w, f in zip(windows, fr)) and all(r is w for r, w in zip(results, windows))
    # key 0 unreadable, key 3 cut one level early, link 2 unreadable
    bad = list(datas)
    bad[0] = bad[0][:5]
    bad[2] = b"\xff\xff" + bad[2][2:]
    bad[3] = levels.late_prefix(bad[3], W, H, C, orc.geometry(W, H).levels - 2)
    windows, results = clips.decode(bad, left, 3, W, H, C, lo, hi)
    assert results[0] is None and results[2] is None and results[3] is clips.UNTOUCHED
    assert windows[0] is left[0] and windows[2] is left[2] and windows[3] is left[3]
    assert (windows[1] == np.clip(left[0].astype(np.int64) + delta.residual(fr[1], fr[0]), lo, hi)).all()
    assert (windows[4] == np.clip(left[3].astype(np.int64) + delta.residual(fr[4], fr[3]), lo, hi)).all()
    assert (windows[1] != fr[1]).any() and (windows[4] != fr[4]).any()


@pytest.mark.parametrize("rng", RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", signed.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_clips_round_trip(wh, C, rng):
    """n = 7, period 3: three clips, the last of one picture."""
    (W, H), (lo, hi) = wh, rng
    n, period = 7, 3
    fr = clips.frames(W, H, C, lo, hi, n)
    assert len(fr) == n and all(f.dtype == delta.dtype_of(lo, hi) and f.min() >= lo and f.max() <= hi for f in fr)
    junk = [np.full_like(fr[0], lo + 1 + i) for i in range(n)]
    windows, results = clips.decode(clips.streams(fr, period), junk, period, W, H, C, lo, hi)
    for i in range(n):
        assert results[i] is windows[i] and windows[i].dtype == fr[0].dtype and (windows[i] == fr[i]).all(), i


@pytest.mark.parametrize("period", [1, 7, 100])
def test_every_picture_a_key_and_one_clip(period):
    """period == 1: plain streams only; period >= n: one key, n - 1 links."""
    W, H, C, lo, hi = 132, 72, 3, 0, 255
    n = 4
    fr = clips.frames(W, H, C, lo, hi, n)
    datas = clips.streams(fr, period)
    keys = [i for i in range(n) if clips.is_key(i, period)]
    assert keys == (list(range(n)) if period == 1 else [0])
    for i in range(n):
        assert datas[i] == (deep.deep_encode(fr[i])[0] if i in keys else delta.stream(fr[i], fr[i - 1])[0])
    windows, _ = clips.decode(datas, [np.zeros_like(fr[0])] * n, period, W, H, C, lo, hi)
    assert all((w == f).all() for w, f in zip(windows, fr))


# ---- segments: lift.hip's k_clips_from_planes restated -------------------------------------------------------------------------------

def kernel_segments(first, count, period):
    """The launch of dwtx_planes_to_pixels_clips: the number of segments the host asks for, and for segment z the kernel's
    [r0, r1) and whether it starts at a key — its arithmetic, line for line."""
    phase = first % period
    lead = period - phase if phase else 0
    nseg = 1 if lead >= count else (1 if lead else 0) + (count - lead + period - 1) // period
    out = []
    for z in range(nseg):
        s = lead + (z - (1 if lead else 0)) * period
        r0, r1 = max(s, 0), min(s + period, count)
        assert r0 < r1, (first, count, period, z)
        out.append((first + r0, first + r1, s >= 0))
    return out


def test_the_kernels_segments_are_the_runs_between_keys():
    """Every group [first, first + count) of stacks of up to 14 windows under every period up to 15: the segments tile the group
    in order, each holds no key but possibly at its start, and only the first can start without one."""
    for period in range(1, 16):
        for first in range(0, 14):
            for count in range(1, 15 - first):
                got = kernel_segments(first, count, period)
                assert got == clips.segments(first, count, period), (first, count, period)
                assert got[0][0] == first and got[-1][1] == first + count
                for k, (a, b, keyed) in enumerate(got):
                    assert keyed == clips.is_key(a, period) and (keyed or k == 0)
                    assert not any(clips.is_key(i, period) for i in range(a + 1, b))
                    assert k == 0 or a == got[k - 1][1]


# ---- the cut key of the GPU clamp fixture -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", delta.RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", signed.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_the_cut_key_meets_every_clamp(wh, C, rng):
    """The block picture of the range, its plain stream cut at 0.6 of its length: the finest level is still reached and at least
    10 % of the samples are clamped at each end (signed.clamps_are_at_work over the shifted range)."""
    (W, H), (lo, hi) = wh, rng
    data, pic = clips.cut_key(W, H, C, lo, hi)
    r = deep.decoded(data, W, H, C)
    assert r is not None and r[0] == orc.geometry(W, H).levels - 1
    below, above, chans = signed.clamp_shares(r[3], C, lo, hi)
    print(wh, C, rng, "below %.3f above %.3f" % (below, above), chans)
    assert below >= 0.10 and above >= 0.10
    got = clips.key_decode(data, W, H, C, lo, hi, pic.dtype)
    assert got is not None and got is not clips.UNTOUCHED and (got != pic).any()


# ---- dwtx_view_clips_check ---------------------------------------------------------------------------------------------------------

def test_clips_check_takes_and_refuses():
    import dwt_amd

    W, H, n = 16, 8, 5
    frame = H * W
    ptr = 1 << 24
    check = dwt_amd.view_clips_check
    stack = DC._fields(W, H, 1, n, W, frame)
    for dst in (False, True):
        # every period from 1 up is taken: every picture a key, clips, one clip (period >= n)
        for period in (1, 2, 3, n, n + 1, 1 << 20):
            assert check(stack, ptr, period, dst=dst) == (0, ""), period
            assert check(stack, ptr, period, sample_bytes=2, dst=dst) == (0, "")
            assert check(stack, ptr, period, sample_bytes=2, signed=True, minval=-1024, maxval=3071, dst=dst) == (0, "")
        # pitched windows, a tile grid, planar and stepped RGB
        assert check(DC._fields(W, H, 1, n, 2 * W, 2 * frame), ptr, 2, dst=dst) == (0, "")
        assert check(DC._fields(W, H, 1, 6, 3 * W + 5, W, cols=3, band_stride=H * (3 * W + 5)), ptr, 4, dst=dst) == (0, "")
        assert check(DC._fields(W, H, 3, n, W, 3 * frame, channel_stride=frame), ptr, 3, dst=dst) == (0, "")
        assert check(DC._fields(W, H, 3, n, 4 * W, 4 * frame, pixel_step=4), ptr, 3, dst=dst) == (0, "")
        # the refusals, each with a text that starts "clips view:"
        for period in (0, -1, -(1 << 20)):
            rc, text = check(stack, ptr, period, dst=dst)
            assert rc == -3 and text.startswith("clips view: period %d" % period), text
        rc, text = check(None, 0, 2, dst=dst)
        assert rc == -3 and text.startswith("clips view: no view"), text
        rc, text = check(stack, ptr, 2, sample_bytes=1, signed=True, dst=dst)
        assert rc == -3 and text.startswith("clips view:") and "1-byte samples" in text and "int16_t" in text, text
        rc, text = check(stack, ptr, 2, sample_bytes=2, minval=-5, dst=dst)
        assert rc == -3 and text.startswith("clips view:") and "without sgn" in text, text
        # what the plain calls refuse of a view: its pixels, its pitch, its sample size
        rc, text = check(stack, 0, 2, dst=dst)
        assert rc == -3 and text.startswith("clips view:"), text
        rc, text = check(DC._fields(W, H, 1, n, W - 1, frame), ptr, 2, dst=dst)
        assert rc == -3 and text.startswith("clips view: row_pitch"), text
        rc, text = check(DC._fields(W, H, 2, n, 2 * W, 2 * frame), ptr, 2, dst=dst)
        assert rc == -3 and text.startswith("clips view:") and "channels 2" in text, text
        rc, text = check(DC._fields(4, 4, 1, n, 4, 16), ptr, 2, dst=dst)
        assert rc == -3 and text.startswith("clips view:") and "4x4" in text, text
        rc, text = check(DC._fields(W, H, 3, n, 2 * W, 3 * frame, pixel_step=2), ptr, 2, dst=dst)
        assert rc == -3 and text.startswith("clips view: pixel_step"), text
    # the period is looked at before the view, the view before anything a decode adds
    rc, text = check(None, 0, 0)
    assert rc == -3 and text.startswith("clips view: period 0"), text
    # decodes read the range and hold the windows apart; encodes do neither
    rc, text = check(stack, ptr, 2, sample_bytes=2, signed=True, minval=100, maxval=50, dst=True)
    assert rc == -3 and text.startswith("clips view:") and "minval < maxval" in text, text
    assert check(stack, ptr, 2, sample_bytes=2, signed=True, minval=100, maxval=50, dst=False) == (0, "")
    rc, text = check(stack, ptr, 2, sample_bytes=1, maxval=100, dst=True)
    assert rc == -3 and text.startswith("clips view: maxval 100"), text
    rc, text = check(DC._fields(W, H, 1, n, W, frame - W), ptr, 2, dst=True)
    assert rc == -3 and text.startswith("clips view: windows overlap"), text
    assert check(DC._fields(W, H, 1, n, W, frame - W), ptr, 2, dst=False) == (0, "")


def test_a_refusal_of_another_call_is_not_said_again():
    """The clips calls say what THEIR view is refused for: a text that an earlier call left behind does not come back."""
    import dwt_amd

    W, H, n = 16, 8, 3
    stack = DC._fields(W, H, 1, n, W, H * W)
    one = DC._fields(W, H, 1, 1, W, 0)
    rc, text = dwt_amd.view_chain_check(stack, one, 1 << 24, 1 << 24, dst=True)
    assert rc == -3 and "meets the key" in text
    rc, text = dwt_amd.view_clips_check(DC._fields(W, H, 1, n, W, H * W), 1 << 24, 2, maxval=70000, sample_bytes=2, dst=True)
    assert rc == -3 and text.startswith("clips view:") and "meets the key" not in text, text


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

def test_clips_entry_points_are_declared_typed_and_exported():
    from dwt_amd import _lib
    import dwt_amd
    import test_abi

    lib = _lib.load()
    declared = test_abi.declared_symbols()
    for name in ("dwtx_encode_view_clips", "dwtx_decode_view_clips", "dwtx_view_clips_check"):
        assert name in declared, f"{name} is not declared in include/dwtx.h"
        assert name in _lib.SYMBOLS, f"{name} is not typed in dwt_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libdwtx.so"
    for fn in (dwt_amd.Context.encode_view_clips, dwt_amd.Context.decode_view_clips):
        assert "period" in inspect.signature(fn).parameters and "key" not in inspect.signature(fn).parameters, fn
    assert callable(dwt_amd.view_clips_check)
