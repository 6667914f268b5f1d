"""Delta chains on the CPU — test infrastructure only.

A chain call (dwtx_encode_view_chain / dwtx_decode_view_chain, include/dwtx.h) is stated by equivalence: n delta calls of one
picture each, call i with window i - 1 as it lies in memory after call i - 1 as its base, and the key for i == 0.  So the
reference is a fold of tests/delta.py's delta_decode over the streams:

    decode   window i = delta_decode(stream i, base) with base = window i - 1 AS DECODED — the clamped samples, not a running
             sum —; a stream that gives None or UNTOUCHED keeps initial[i], what the caller left in the window, and that is
             the next picture's base.

Also here: the pictures of tests/test_chain_cpu.py and tests/test_chain_gpu.py — runs of successor frames, full-range runs
whose residuals leave int16 — and the clamp fixture, a chain of cut streams between two block pictures in which every link
meets every clamp and a wrong base shows in a quarter of the samples or more."""
import numpy as np

import deep
import delta
import orc

UNTOUCHED = delta.UNTOUCHED
CLAMP_CUTS = (0.33, 0.6, 0.33, 0.6)     # of each residual stream's length, link by link (delta.CUTS, twice)
assert set(CLAMP_CUTS) == set(delta.CUTS)


def decode(datas, key, initial, W, H, C, minval, maxval):
    """Streams (bytes) of a chain's residuals, the key [H, W, C] and the windows' contents before the call -> (the windows after
    it, the per-link results: a picture, None or UNTOUCHED)."""
    assert len(datas) == len(initial)
    base, windows, links = key, [], []
    for data, was in zip(datas, initial):
        r = delta.delta_decode(data, base, W, H, C, minval, maxval)
        links.append(r)
        base = was if r is None or r is UNTOUCHED else r
        windows.append(base)
    return windows, links


# ---- pictures ------------------------------------------------------------------------------------------------------------------

_frames = {}


def frames(W, H, C, minval, maxval, n, seed=2):
    """n + 1 frames of the range, each the successor of the one before: fresh noise of -2 .. 2 on every sample and a 40 x 32
    block that moves on by a few pixels (tests/test_delta_gpu.py's chain)."""
    key = (W, H, C, minval, maxval, n, seed)
    if key not in _frames:
        rng = np.random.default_rng(75 + seed)
        out = [delta.successor(W, H, C, minval, maxval, seed)[1]]
        for i in range(n):
            f = out[-1].astype(np.int64)
            g = f + rng.integers(-2, 3, f.shape)
            g[20 + i:52 + i, 30 + 2 * i:70 + 2 * i] = f[18:50, 27:67]
            out.append(np.clip(g, minval, maxval).astype(out[0].dtype))
        _frames[key] = out
    return _frames[key]


def full_range_frames(W, H, sgn, n):
    """n + 1 gray frames over the whole range of uint16 or int16 that alternate between a rising and a falling picture
    (delta.full_range_pair): every residual leaves int16."""
    pairs = [delta.full_range_pair(W, H, sgn, s) for s in range((n + 2) // 2)]
    out = []
    for S, B in pairs:
        out += [B, S]
    return out[:n + 1]


def streams(fr):
    """The residual streams of frames fr[1:], each against the frame before it."""
    return [delta.stream(fr[i + 1], fr[i])[0] for i in range(len(fr) - 1)]


# ---- the clamp fixture ---------------------------------------------------------------------------------------------------------

def clamp_fixture(W, H, C, minval, maxval):
    """-> (key, the four cut residual streams, the four true frames).  The key is the second block picture of delta.clamp_pair,
    the frames alternate between the first and the second: every residual's samples are -R, 0 and R, and a stream cut at a
    third or at 0.6 of its length leaves a decode that meets every clamp."""
    S, B = delta.clamp_pair(W, H, C, minval, maxval)
    true = [S, B, S, B]
    prev = [B, S, B, S]
    datas = []
    for t, p, cut in zip(true, prev, CLAMP_CUTS):
        data = delta.stream(t, p)[0]
        datas.append(data[:int(len(data) * cut)])
    return B, datas, true


def clamp_fixture_report(W, H, C, minval, maxval):
    """What tests/test_chain_cpu.py holds the fixture to, link by link with the RUNNING decoded base: (reaches the finest level,
    delta.clamps_are_at_work, delta.clamp_shares, the share of samples that differ from the decode onto the TRUE previous
    frame)."""
    key, datas, true = clamp_fixture(W, H, C, minval, maxval)
    base, out = key, []
    T = orc.geometry(W, H).levels
    for i, data in enumerate(datas):
        r = deep.decoded(data, W, H, C)
        assert r is not None
        finest = r[0] == T - 1
        work = delta.clamps_are_at_work(r[3], base, W, H, C, minval, maxval)
        shares = delta.clamp_shares(r[3], base, C, minval, maxval)
        got = delta.delta_pixels(r[3], base, C, minval, maxval)
        other = delta.delta_pixels(r[3], true[i - 1] if i else key, C, minval, maxval)
        out.append((finest, work, shares, float((got != other).mean())))
        base = got
    return out
