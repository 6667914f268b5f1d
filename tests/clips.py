"""Clip stacks on the CPU — test infrastructure only.

A clips call (dwtx_encode_view_clips / dwtx_decode_view_clips, include/dwtx.h) is one stack of n windows in which window i with
i % period == 0 is a KEY, coded as itself, and every other window a LINK, coded against window i - 1.  The decode is stated by
equivalence, a walk over i = 0 .. n - 1, and that walk is the reference here:

    key      the plain decode of stream i alone (deep.decoded, then tests/signed.py's clamps for [minval, maxval] — with
             minval = 0 deep.to_pixels') if the stream is readable AND supports the whole picture; else the window keeps
             initial[i], what the caller left there: None for an unreadable stream, UNTOUCHED for one that stops before its
             finest level — the clips call writes whole pictures only, a cut key's corner is NOT written.
    link     tests/delta.py's delta_decode of stream i alone onto window i - 1 AS IT LIES THERE at that moment — the clamped
             samples that were decoded, or what the caller left —; None and UNTOUCHED keep initial[i], and the next link
             takes that.

    encode   a key's stream is the plain stream of its picture (deep.deep_encode), a link's delta.stream(window i, window i - 1).

The pictures are tests/chain.py's frames."""
import numpy as np

import chain
import deep
import delta
import orc
import signed

UNTOUCHED = delta.UNTOUCHED


def is_key(i, period):
    return i % period == 0


def key_pixels(img, C, minval, maxval, dtype):
    """The inverse transform's output [H, W, C] of a plain picture -> its samples in `dtype`: signed.clamp_pixels without its
    int16 cast (a uint16 picture reaches 65535), held to it wherever the range fits, and to deep.to_pixels where minval is 0."""
    a = img.astype(np.int64)
    R = maxval - minval
    if C == 1:
        out = np.clip(a, minval, maxval)
    else:
        ycc = np.stack([np.clip(a[..., 0], minval, maxval), np.clip(a[..., 1], -R, R), np.clip(a[..., 2], -R, R)], -1)
        out = np.clip(deep.ycocg2rgb(ycc, None), minval, maxval)
    if minval >= -32768 and maxval <= 32767:
        assert (out == signed.clamp_pixels(img, C, minval, maxval)).all()
    if minval == 0:
        assert (out == deep.to_pixels(img, C, maxval)).all()
    return out.astype(dtype)


def key_decode(data, W, H, C, minval, maxval, dtype):
    """.dwt bytes of a plain picture (or a prefix) -> the picture in `dtype`, None where decode.c would exit 1, UNTOUCHED where
    the stream supports less than W x H."""
    r = deep.decoded(data, W, H, C)
    if r is None:
        return None
    if r[0] != orc.geometry(W, H).levels - 1:
        return UNTOUCHED
    return key_pixels(r[3], C, minval, maxval, dtype)


def decode(datas, initial, period, W, H, C, minval, maxval):
    """The streams (bytes) of a clip stack and the windows' contents before the call -> (the windows after it, the per-window
    results: a picture, None or UNTOUCHED)."""
    assert len(datas) == len(initial) and period >= 1
    windows, results = [], []
    for i, (data, was) in enumerate(zip(datas, initial)):
        if is_key(i, period):
            r = key_decode(data, W, H, C, minval, maxval, was.dtype)
        else:
            r = delta.delta_decode(data, windows[i - 1], W, H, C, minval, maxval)
        results.append(r)
        windows.append(was if r is None or r is UNTOUCHED else r)
    return windows, results


_plain = {}


def plain_stream(pic, capacity=0):
    """-> (.dwt bytes, orc.Stats) of a picture coded as itself, made once."""
    key = (pic.tobytes(), pic.shape, str(pic.dtype), capacity)
    if key not in _plain:
        _plain[key] = deep.deep_encode(pic, capacity)
    return _plain[key]


def stream(fr, i, period, capacity=0):
    """-> (.dwt bytes, orc.Stats) of window i of the stack `fr`."""
    return plain_stream(fr[i], capacity) if is_key(i, period) else delta.stream(fr[i], fr[i - 1], capacity)


def streams(fr, period):
    return [stream(fr, i, period)[0] for i in range(len(fr))]


def cut_key(W, H, C, minval, maxval, cut=0.6):
    """-> (the prefix at `cut` of the plain stream of a block picture of the range — the second of delta.clamp_pair, the key of
    chain.clamp_fixture —, that picture): every sample at one of the range's ends, so that a decode that lost planes meets the
    plain pictures' clamps (tests/test_clips_cpu.py holds it to that)."""
    pic = delta.clamp_pair(W, H, C, minval, maxval)[1]
    data = plain_stream(pic)[0]
    return data[:int(len(data) * cut)], pic


def frames(W, H, C, minval, maxval, n, seed=2):
    """n frames of a stack: chain.frames' run of successors (which has n + 1 for n links)."""
    return chain.frames(W, H, C, minval, maxval, n - 1, seed)


def segments(first, count, period):
    """The segments of a group of windows [first, first + count), as lift.hip's k_clips_from_planes cuts it: maximal runs with no
    key except possibly at their start -> [(start, stop, keyed)] in windows of the stack."""
    out, i = [], first
    while i < first + count:
        j = i + 1
        while j < first + count and not is_key(j, period):
            j += 1
        out.append((i, j, is_key(i, period)))
        i = j
    return out
