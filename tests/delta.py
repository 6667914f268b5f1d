"""Delta views on the CPU — test infrastructure only.

A delta call (dwtx_encode_view_delta / dwtx_decode_view_delta, include/dwtx.h) codes the integer picture D = S - B: the bytes
are tests/deep.py's composition of the oracle's depth-agnostic stages on D, which never asked where its integers came from.
What is new is the decoder's end, restated here:

    decode   deep.decoded; a stream that is unreadable gives None, one that stops before its finest level "untouched" (a
             coarse residual has no base of its size).  Else, with R = maxval - minval, the residual d is the inverse
             transform's output under tests/signed.py's clamps for the range [-R, R] — gray and Y to [-R, R], Co and Cg to
             [-2R, 2R], every sample of d to [-R, R] — and the picture is min(max(B + d, minval), maxval).

Also here: the pictures of tests/test_delta_cpu.py and tests/test_delta_gpu.py — successor frames of deep.smooth_noise
pictures, full-range pairs whose residuals leave int16 — and the cut streams whose decodes meet every clamp, with the
condition those must fulfil."""
import numpy as np

import deep
import orc
import signed

RANGES = [(0, 255), (0, 4095), (-1024, 3071)]     # uint8, uint16 (12 bits), int16 (a CT slice's)
SHAPES = signed.SHAPES                            # one wide level, general conversions, two wide levels
CUTS = signed.CUTS                                # of a stream's length: the clamp fixtures
UNTOUCHED = "untouched"


def dtype_of(minval, maxval):
    return np.int16 if minval < 0 else np.uint8 if maxval <= 255 else np.uint16


def residual(S, B):
    """The integer picture a delta encode codes."""
    assert S.shape == B.shape
    return S.astype(np.int64) - B.astype(np.int64)


def clamp_residual(img, C, R):
    """signed.clamp_pixels for the range [-R, R] without its int16 cast (R reaches 65535): int64 [..., C]."""
    a = img.astype(np.int64)
    if C == 1:
        return np.clip(a, -R, R)
    ycc = np.stack([np.clip(a[..., 0], -R, R), np.clip(a[..., 1], -2 * R, 2 * R), np.clip(a[..., 2], -2 * R, 2 * R)], -1)
    return np.clip(deep.ycocg2rgb(ycc, None), -R, R)


def delta_pixels(img, B, C, minval, maxval):
    """The inverse transform's output [H, W, C] of a residual and the base -> the picture in the base's dtype."""
    R = maxval - minval
    d = clamp_residual(img, C, R)
    if R <= 32767:
        assert (d == signed.clamp_pixels(img, C, -R, R)).all()
    return np.clip(B.astype(np.int64) + d, minval, maxval).astype(B.dtype)


def delta_decode(data, B, W, H, C, minval, maxval):
    """.dwt bytes of a residual (or a prefix) and the base [H, W, C] -> the picture in the base's dtype, None where decode.c
    would exit 1, UNTOUCHED where the stream supports less than W x H."""
    r = deep.decoded(data, W, H, C)
    if r is None:
        return None
    if r[0] != orc.geometry(W, H).levels - 1:
        return UNTOUCHED
    return delta_pixels(r[3], B, C, minval, maxval)


# ---- pictures ------------------------------------------------------------------------------------------------------------------

_pairs = {}


def successor(W, H, C, minval, maxval, seed=0):
    """-> (S, B): B a smooth + noise picture of the range, S its successor frame — fresh noise of -2 .. 2 on every sample and
    a 40 x 32 block that has moved by a few pixels —, both in the range's dtype."""
    key = (W, H, C, minval, maxval, seed)
    if key not in _pairs:
        R = maxval - minval
        rng = np.random.default_rng(1000 + seed)
        B = deep.smooth_noise(W, H, C, R, seed).astype(np.int64)
        S = B + rng.integers(-2, 3, B.shape)
        y0, x0 = H // 3, W // 4
        dy, dx = 2 + seed % 3, 3 + seed % 4
        S[y0 + dy:y0 + dy + 32, x0 + dx:x0 + dx + 40] = B[y0:y0 + 32, x0:x0 + 40]
        S = np.clip(S, 0, R)
        dt = dtype_of(minval, maxval)
        _pairs[key] = ((S + minval).astype(dt), (B + minval).astype(dt))
    return _pairs[key]


def full_range_pair(W, H, sgn, seed=0):
    """-> (S, B), gray, uint16 or int16 over the type's whole range: a rising and a falling picture, so that the residual
    runs from about -65535 to 50000 — outside int16 — while its details stay small."""
    key = (W, H, "full", sgn, seed)
    if key not in _pairs:
        S = deep.smooth_noise(W, H, 1, 65535, seed + 1).astype(np.int64)
        B = 65535 - deep.smooth_noise(W, H, 1, 65535, seed + 2).astype(np.int64)
        lo = -32768 if sgn else 0
        dt = np.int16 if sgn else np.uint16
        _pairs[key] = ((S + lo).astype(dt), (B + lo).astype(dt))
    return _pairs[key]


def noise_pair(W, H, sgn):
    """Two full-range noise pictures: a residual of 18 planes, which every encoder refuses."""
    lo = -32768 if sgn else 0
    dt = np.int16 if sgn else np.uint16
    return tuple((deep.noise(W, H, 1, 65535, s).astype(np.int64) + lo).astype(dt) for s in (4, 5))


_streams = {}


def stream(S, B, capacity=0):
    """-> (.dwt bytes, orc.Stats) of the residual, made once."""
    key = (S.tobytes(), B.tobytes(), S.shape, str(S.dtype), capacity)
    if key not in _streams:
        _streams[key] = deep.deep_encode(residual(S, B), capacity)
    return _streams[key]


# ---- the clamp fixtures --------------------------------------------------------------------------------------------------------

def clamp_pair(W, H, C, minval, maxval):
    """-> (S, B): two block pictures of the range, every sample at one of its ends: the residual's samples are -R, 0 and R."""
    R = maxval - minval
    dt = dtype_of(minval, maxval)
    return tuple((deep.blocks(W, H, C, R, seed).astype(np.int64) + minval).astype(dt) for seed in (5, 3))


def cut_fixture(W, H, C, minval, maxval, cut):
    """-> (prefix of the residual's stream at `cut` of its length, B)."""
    S, B = clamp_pair(W, H, C, minval, maxval)
    data = stream(S, B)[0]
    return data[:int(len(data) * cut)], B


def clamp_shares(img, B, C, minval, maxval):
    """What the clamps find in an inverse transform's output [H, W, C]: (share of the final samples below minval, above
    maxval, share of the residual's samples outside [-R, R] after the colour transform, [share of Y outside [-R, R], of Co
    and of Cg outside [-2R, 2R]] — empty for gray)."""
    a = img.astype(np.int64)
    R = maxval - minval
    if C == 1:
        d0, chans = a, []
    else:
        chans = [float((np.abs(a[..., 0]) > R).mean())] + [float((np.abs(a[..., c]) > 2 * R).mean()) for c in (1, 2)]
        ycc = np.stack([np.clip(a[..., 0], -R, R), np.clip(a[..., 1], -2 * R, 2 * R), np.clip(a[..., 2], -2 * R, 2 * R)], -1)
        d0 = deep.ycocg2rgb(ycc, None)
    out = B.astype(np.int64) + np.clip(d0, -R, R)
    return float((out < minval).mean()), float((out > maxval).mean()), float((np.abs(d0) > R).mean()), chans


def clamps_are_at_work(img, B, W, H, C, minval, maxval):
    """The condition every clamp fixture is held to: full size, at least 10 % of the final samples clamped at each of minval
    and maxval, at least 10 % of the residual's samples outside [-R, R], and for RGB each of Y, Co and Cg outside its clamp
    on at least 0.3 % of the samples."""
    below, above, outside, chans = clamp_shares(img, B, C, minval, maxval)
    return img.shape == (H, W, C) and below >= 0.10 and above >= 0.10 and outside >= 0.10 and all(s >= 0.003 for s in chans)
