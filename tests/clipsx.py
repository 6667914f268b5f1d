"""Clip stacks with a crop per clip and float windows on the CPU — test infrastructure only.

dwtx_decode_view_clips_crop (include/dwtx.h) is stated by equivalence, and both of its walks are restated here from pieces that
exist: deep.decoded gives the inverse transform's output of a stream, clips.key_pixels turns the CROPPED output of a key into
samples, delta.delta_pixels the cropped output of a link and the cropped base — both are per pixel, so cropping first is exact
(tests/test_clips_crop_cpu.py holds that to the slice of clips.decode's full-size result) — and floats.reference gives the bits of
a float window.

    integer walk   clips.decode on crop-sized windows: a key that is readable and whole receives the crop of its plain picture,
                   a link clamp(window i - 1 as it lies there + crop of d); None and UNTOUCHED keep what the caller left.
    float walk     carries its own INTEGER running picture and a flag per clip: a whole key sets the flag and is written; a key
                   that is not whole clears it; a link is written only if the flag is set and its own stream is readable and
                   whole, else it clears the flag — a break ends the clip, and the destination is never read.

Clip k is windows [k * period, (k + 1) * period) and has ONE origin; expand() spells the origins out per picture, as the host
does for dwtx_inv_crop.  The host's launch arithmetic for float groups (codec.hip, decode_device: float_run) is restated in
launches()."""
import numpy as np

import clips
import deep
import delta
import floats
import orc

UNTOUCHED = clips.UNTOUCHED


def nclips(n, period):
    return -(-n // period)


def expand(origins, n, period):
    """per-clip origins (None: all (0, 0)) -> one (x0, y0) per picture"""
    if origins is None:
        return [(0, 0)] * n
    assert len(origins) == nclips(n, period)
    return [tuple(origins[i // period]) for i in range(n)]


_decoded = {}


def cropped(data, W, H, C, x0, y0, cw, ch):
    """.dwt bytes -> the crop of the inverse transform's output [ch, cw, C], None where decode.c would exit 1, UNTOUCHED where
    the stream supports less than W x H.  The decode of a stream is made once."""
    key = (data, W, H, C)
    if key not in _decoded:
        r = deep.decoded(data, W, H, C)
        _decoded[key] = None if r is None else UNTOUCHED if r[0] != orc.geometry(W, H).levels - 1 else r[3]
    img = _decoded[key]
    if img is None or img is UNTOUCHED:
        return img
    assert 0 <= x0 <= W - cw and 0 <= y0 <= H - ch
    return img[y0:y0 + ch, x0:x0 + cw]


def decode(datas, initial, period, W, H, C, minval, maxval, cw, ch, origins=None):
    """The integer walk.  initial: the crop-sized windows' contents before the call -> (the windows after it, the per-window
    results: a picture, None or UNTOUCHED)."""
    at = expand(origins, len(datas), period)
    windows, results = [], []
    for i, (data, was) in enumerate(zip(datas, initial)):
        img = cropped(data, W, H, C, *at[i], cw, ch)
        if img is None or img is UNTOUCHED:
            r = img
        elif clips.is_key(i, period):
            r = clips.key_pixels(img, C, minval, maxval, was.dtype)
        else:
            r = delta.delta_pixels(img, windows[i - 1], C, minval, maxval)
        results.append(r)
        windows.append(was if r is None or r is UNTOUCHED else r)
    return windows, results


def decode_float(datas, period, W, H, C, minval, maxval, cw, ch, origins=None):
    """The float walk's INTEGERS -> (per window: the clamped integer picture [ch, cw, C] (int64) that is written, or None for a
    window that stays untouched; per window: why — "key", "link", or the break: "cut key", "unreadable key", "unreadable
    link", "cut link", "dead")."""
    at = expand(origins, len(datas), period)
    written, why = [], []
    run, live = None, False
    for i, data in enumerate(datas):
        img = cropped(data, W, H, C, *at[i], cw, ch)
        key = clips.is_key(i, period)
        whole = img is not None and img is not UNTOUCHED
        if key and whole:
            run, live = clips.key_pixels(img, C, minval, maxval, np.int64), True
            why.append("key")
        elif key:
            live = False
            why.append("unreadable key" if img is None else "cut key")
        elif live and whole:
            run = delta.delta_pixels(img, run, C, minval, maxval)
            why.append("link")
        else:
            why.append("dead" if not live else "unreadable link" if img is None else "cut link")
            live = False
        written.append(run if live else None)
    return written, why


def float_bits(written, kind, scale, bias, order="rgb"):
    """decode_float's pictures -> the bits of each written window as they lie in memory (None stays None)"""
    return [None if v is None else floats.reference(v, kind, scale, bias, order) for v in written]


def launches(groups, whole, n, period):
    """The conversion launches of a float call.  groups: the (first, count) of every call of decode_device's `finish` that reaches
    the conversion, in ascending order (a uniform part: the part; the fallback: one window each, whole ones only); whole[i]:
    window i's stream is readable and supports the whole picture -> [(first, count, reads_carry, writes_carry, slot_read,
    slot_written)] of the launches that are made: a first segment that starts mid-clip on a dead clip is dropped, a live one
    reads the carry picture the launch before wrote, and a last segment that ends mid-clip writes the OTHER one."""
    out, seen, live, last = [], 0, False, 0
    for first, count in groups:
        assert first >= seen and all(whole[first:first + count])
        if seen < first:
            live = False
        seen = end = first + count
        lead = (period - first % period) % period
        reads = False
        if lead and not live:
            skip = min(lead, count)
            first, count = first + skip, count - skip
        elif lead:
            reads = True
        if count < 1:
            continue
        writes = end < n and end % period != 0
        slot_read = last if reads else None
        if writes:
            last ^= 1
        out.append((first, count, reads, writes, slot_read, last if writes else None))
        live = True
    return out


def groups_of(parts, whole):
    """deep.decoder_parts' ranges and the windows' whole flags -> launches()' groups: a part whose every window is whole is ONE
    group (the test streams of one call are encoded alike: a uniform part); any other part falls back to one group per whole
    window."""
    out = []
    for p in parts:
        if all(whole[i] for i in p):
            out.append((p[0], len(p)))
        else:
            out += [(i, 1) for i in p if whole[i]]
    return out
