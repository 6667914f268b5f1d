"""Signed 16-bit samples on the CPU — test infrastructure only.

A signed picture is coded as the integers it holds: tests/deep.py's composition of the oracle's depth-agnostic stages
(deep_encode: orc.forward -> orc.linearize -> orc.encode_lin, after YCoCg-R for colour, which image.h:53-65 makes
reversible on any int) never asked for a sign of its input.  What is new is the two ends, and they are restated here:

    decode   deep.decoded, then the clamps of image.h:41-43 and pnm.h:108 for a range [minval, maxval] with
             R = maxval - minval: gray and Y to [minval, maxval], Co and Cg to [-R, R], every output sample to
             [minval, maxval] — with minval = 0 deep.to_pixels'.
    quantise a float source's integers: rint(fl32(fl32(x * scale) + bias)), ties to even, NaN -> 0, clamped to
             [minval, maxval] — with minval = 0 tests/quant.py's.

Also here: the pictures of tests/test_signed_cpu.py and tests/test_signed_gpu.py (deep.py's generators over R, shifted by
minval) and the cut streams whose decodes meet every clamp, with the condition those must fulfil."""
import numpy as np

import deep
import orc

RANGES = [(-1024, 3071), (-2048, 2047)]          # a CT slice's, a residual's
FULL = (-32768, 32767)
SHAPES = [(132, 72), (263, 135), (520, 264)]     # fused with one wide level, general conversions, two wide levels
CUTS = (0.33, 0.6)                               # of a stream's length: the clamp fixtures


def clamp_pixels(img, C, minval, maxval):
    """The inverse transform's output [..., C] (Y, Co, Cg for C == 3) -> int16 samples: image.h:39-51 and pnm.h:108 with the
    range's bounds where those have 0 and 255."""
    a = img.astype(np.int64)
    R = maxval - minval
    if C == 1:
        return np.clip(a, minval, maxval).astype(np.int16)
    ycc = np.stack([np.clip(a[..., 0], minval, maxval), np.clip(a[..., 1], -R, R), np.clip(a[..., 2], -R, R)], -1)
    return np.clip(deep.ycocg2rgb(ycc, None), minval, maxval).astype(np.int16)


def signed_decode(data, W, H, C, minval, maxval, pixels_max=-1):
    """.dwt bytes (or a prefix) -> int16 [h, w, C] with the clamps of the range, or None where decode.c would exit 1."""
    r = deep.decoded(data, W, H, C, pixels_max)
    return None if r is None else clamp_pixels(r[3], C, minval, maxval)


def quantise(x, scale, bias, minval, maxval):
    """float array [..., C] (any float type numpy widens exactly) -> the int64 samples dwtx_encode_view_signed codes: scale and
    bias per colour (a number, or C of them), two float32 roundings, ties to even, NaN -> 0 before the clamp."""
    x = np.asarray(x).astype(np.float32)
    s = np.broadcast_to(np.asarray(scale, dtype=np.float32), x.shape[-1:])
    b = np.broadcast_to(np.asarray(bias, dtype=np.float32), x.shape[-1:])
    with np.errstate(invalid="ignore", over="ignore"):
        m = (x * s).astype(np.float32)
        r = (m + b).astype(np.float32)
        q = np.rint(r)
    q = np.where(np.isnan(q), np.float32(0), q)
    return np.clip(q, minval, maxval).astype(np.int64)


def _shift(pic, minval):
    out = pic.astype(np.int64) + minval
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16)


def smooth_noise(W, H, C, minval, maxval, seed=0):
    return _shift(deep.smooth_noise(W, H, C, maxval - minval, seed), minval)


def blocks(W, H, C, minval, maxval, seed=3):
    return _shift(deep.blocks(W, H, C, maxval - minval, seed), minval)


def noise(W, H, C, minval, maxval, seed=0):
    return _shift(deep.noise(W, H, C, maxval - minval, seed), minval)


def zero_crossing(W, H, C):
    """A gentle ramp through zero, a few counts of noise: 5-6 planes as signed integers; the same bytes read as uint16 jump by
    65535 at every crossing."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[:H, :W]
    ramp = ((x + 2 * y) % 97 - 48)[..., None] + np.arange(C) * 3
    return (ramp + rng.integers(-2, 3, (H, W, C))).astype(np.int16)


_streams = {}


def stream(kind, W, H, C, minval, maxval, seed=0):
    """-> (picture int16 [H, W, C], .dwt bytes, orc.Stats) of generator `kind` ("smooth_noise", "blocks", "noise"), made once."""
    key = (kind, W, H, C, minval, maxval, seed)
    if key not in _streams:
        pic = globals()[kind](W, H, C, minval, maxval, seed)
        _streams[key] = (pic,) + deep.deep_encode(pic)
    return _streams[key]


def cut_fixture(W, H, C, minval, maxval, cut):
    """The prefix of the blocks picture's stream at `cut` of its length: a decode that every clamp of the range acts on."""
    data = stream("blocks", W, H, C, minval, maxval, 3)[1]
    return data[:int(len(data) * cut)]


def clamp_shares(img, C, minval, maxval):
    """What the clamps find in an inverse transform's output [h, w, C] before any of them: (share of the final samples below
    minval, share above maxval, [share of Y outside [minval, maxval], of Co and of Cg outside [-R, R]] — empty for gray)."""
    a = img.astype(np.int64)
    R = maxval - minval
    out = deep.ycocg2rgb(a, None) if C == 3 else a
    chans = [] if C == 1 else [float(((a[..., 0] < minval) | (a[..., 0] > maxval)).mean())] + \
        [float((np.abs(a[..., c]) > R).mean()) for c in (1, 2)]
    return float((out < minval).mean()), float((out > maxval).mean()), chans


def clamps_are_at_work(img, W, H, C, minval, maxval):
    """The condition every clamp fixture is held to: full size, at least 10 % of the samples below minval, at least 10 % above
    maxval, and for RGB each of Y, Co and Cg outside its clamp on at least 3 % of the samples."""
    below, above, chans = clamp_shares(img, C, minval, maxval)
    return img.shape == (H, W, C) and below >= 0.10 and above >= 0.10 and all(s >= 0.03 for s in chans)
