"""Decodes that stop at every level — test infrastructure only, CPU only: the streams and batches of
tests/test_levels_cpu.py and tests/test_levels_gpu.py.

A .dwt that ends early, or a decode with a PIXELS cap, gives the picture of widths / heights[info.level + 1]
(decode.c:251-254), and in the library that size — not the stream's W x H — picks everything after the token walk: the
kernel family that writes the pixels, whether a batch part is finished in one go, whether its finest rings were fused.
The prefixes that stop a decode at a given level are a few dozen to a few hundred bytes long; they are found here with
the oracle (orc.decode_stage), never with the library.

Levels are counted as decode.c counts them: info.level == l means ring levels 0 .. l were reached, the picture is
widths[l + 1] x heights[l + 1]; -1 is the root image alone.  A "size index" k = level + 1 runs from 0 (root) to
`levels` (the whole picture)."""
import deep
import orc

# (W, H): 263x135 is general whole and wide at 132x68; 511x259 is general whole, wide at 256x130 and 128x65 (only H above the
# tail), tail at 64x33; 520x264 is wide whole, on a strip edge at 260x132, general at 130x66 and 65x33; 256x256 is wide at
# every size down to 128 and the tail from 64x64
SHAPES = [(263, 135), (511, 259), (520, 264), (256, 256)]
M16 = 4095          # maxval of the deep pictures
QUAD = 4            # samples of a lane of the wide kernels: widths, origins and strides must be multiples (dwtx_pixels::wide)
TAIL_MAX = 64       # no side above it: the LDS tail writes the picture (lift.hip)
WHOLE = None        # a row's stop: the whole stream


# ---- geometry and families -------------------------------------------------------------------------------------------

def levels_of(W, H):
    return orc.geometry(W, H).levels


def sizes(W, H):
    """[(ow, oh)] by size index 0 .. levels"""
    g = orc.geometry(W, H)
    return [(g.widths[k], g.heights[k]) for k in range(g.levels + 1)]


def family(ow, oh, on_grid):
    """Which kernels write an ow x oh picture (dwtx_pixels_ok, dwtx_internal.h): "wide" — the inverse transform's last
    level writes the pixels itself: ow a multiple of 4, a side above 64 and every row of every window on the quad grid of
    its sample type (on_grid); "tail" — no side above 64: one workgroup in LDS; else "general": int32 planes and the general
    conversion.  (Off the grid a picture without a side above 64 is still transformed by the tail.)"""
    if ow <= TAIL_MAX and oh <= TAIL_MAX:
        return "tail"
    return "wide" if ow % QUAD == 0 and on_grid else "general"


def on_grid(L, is16=False, floats=False):
    """Does a layout (tests/test_views_gpu.py's Layout: off, shape [.., H, W, C], strides in samples) put every row of every
    window — of every plane — on the quad grid, and is it one the wide kernels take at all?  The origin and every stride above
    the pixel are multiples of 4 samples; planar pixels (column stride 1): the channel stride too; pixels with a step: 8-bit
    RGB in 4-sample pixels only; float samples: gray and planar RGB only."""
    Cn = L.shape[-1]
    col, ch = L.strides[-2], L.strides[-1]
    planar = Cn == 3 and col == 1
    stepped = not planar and col != Cn
    if L.off % QUAD or any(s % QUAD for s in L.strides[:-2]) or (planar and ch % QUAD):
        return False
    if stepped and not (col == 4 and Cn == 3 and not is16 and not floats):
        return False
    return not (floats and Cn == 3 and not planar)


# ---- pictures, streams, prefixes -----------------------------------------------------------------------------------------

_streams, _levels, _prefix = {}, {}, {}


def stream(W, H, Cn, is16, i):
    """Picture i of a shape as a whole .dwt: orc.synth's for bytes; for deep pixels (maxval 4095) deep.smooth_noise's — or,
    where that stream passes a level within one byte (its coarse rings are nearly empty: every deep RGB picture of 263x135 and
    most gray ones), deep.blocks's, whose streams stop at every level.  The oracle alone decides."""
    key = (W, H, Cn, is16, i)
    if key not in _streams:
        if not is16:
            _streams[key] = orc.encode(orc.synth(W, H, Cn, i, 0))[0]
        else:
            data = deep.deep_encode(deep.smooth_noise(W, H, Cn, M16, seed=i))[0]
            if any(_shortest(data, W, H, Cn, l) is None for l in range(levels_of(W, H))):
                data = deep.deep_encode(deep.blocks(W, H, Cn, M16, seed=i))[0]
            _streams[key] = data
    return _streams[key]


def level_at(data, W, H, Cn, k):
    """The level the oracle reaches on data[:k]; -2: unreadable."""
    key = (data, k)
    if key not in _levels:
        r = orc.decode_stage(data[:k], W, H, Cn)
        _levels[key] = -2 if r is None else r[1]
    return _levels[key]


def _shortest(data, W, H, Cn, l):
    """The length of the shortest prefix whose level is l; None if the stream passes level l within one byte."""
    key = (data, l)
    if key not in _prefix:
        lo, hi = 6, 8   # (6 bytes are the header alone: unreadable)
        while level_at(data, W, H, Cn, hi) < l:
            assert hi < len(data), f"the whole stream does not reach level {l}"
            lo, hi = hi, min(2 * hi, len(data))
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if level_at(data, W, H, Cn, mid) < l:
                lo = mid
            else:
                hi = mid
        _prefix[key] = hi if level_at(data, W, H, Cn, hi) == l else None
    return _prefix[key]


def prefix_for_level(data, W, H, Cn, l):
    """The shortest prefix of `data` whose oracle level is l (-1 .. levels - 1).  The level only grows with the length, so:
    double a bound until it reaches l, then bisect."""
    k = _shortest(data, W, H, Cn, l)
    assert k is not None, f"no prefix stops at level {l}: the stream passes it within one byte"
    return data[:k]


def late_prefix(data, W, H, Cn, l):
    """The longest prefix whose level is still l: one byte short of level l + 1, or of the whole stream."""
    if l == levels_of(W, H) - 1:
        return data[:-1]
    return data[:len(prefix_for_level(data, W, H, Cn, l + 1)) - 1]


# ---- the cases -------------------------------------------------------------------------------------------------------------

def plan(W, H, n):
    """-> [(name, stops, cap)]: per row a stop — WHOLE, ("first", l) or ("late", l) — and the size index the batch is capped at
    (None: no cap).  Geometry alone; level_cases makes the streams from it."""
    T = levels_of(W, H)
    whole = [WHOLE] * n
    first = lambda l: ("first", l) if l < T else WHOLE   # noqa: E731
    cases = [("cap %d" % k, whole, k) for k in range(T + 1)]
    cases += [("stop %d" % l, [first(l)] * n, None) for l in range(T)]
    # even rows one byte short of the next level, odd rows the shortest: one level, different missing[]
    cases += [("stop %d late" % l, [("late", l) if i % 2 == 0 else first(l) for i in range(n)], None) for l in range(T)]
    stairs = [first(i % (T + 1)) for i in range(n)]
    cases += [("stairs", stairs, None), ("stairs capped", stairs, T // 2)]
    short = first(T - 2)
    cases += [("one short", whole[:-1] + [short], None), ("short first", [short] + whole[:-1], None)]
    return cases


def size_index(W, H, stop):
    """The size index of a row that is decoded without a cap.  (Under a cap the picture may be smaller than the cap's size: the
    walk of decode.c:198-243 stops at the first segment of a level beyond the cap, which may come before a channel with fewer
    planes has had any — the oracle knows, a plan does not.)"""
    return levels_of(W, H) if stop is WHOLE else stop[1] + 1


def level_cases(W, H, Cn, is16, n, names=None):
    """-> [(name, rows, pixels_max)] as V.check_decode and check_float take them: row i is picture i's stream, cut as plan()
    says.  names: only the cases whose name starts with one of these."""
    g = orc.geometry(W, H)
    out = []
    for name, stops, cap in plan(W, H, n):
        if names is not None and not any(name.startswith(p) for p in names):
            continue
        rows = []
        for i, stop in enumerate(stops):
            data = stream(W, H, Cn, is16, i)
            if stop is WHOLE:
                rows.append(data)
            elif stop[0] == "first":
                rows.append(prefix_for_level(data, W, H, Cn, stop[1]))
            else:
                rows.append(late_prefix(data, W, H, Cn, stop[1]))
        out.append((name, rows, -1 if cap is None else g.pixels[cap]))
    return out


def families(W, H, n, grid_ok, names=None):
    """{(family, ow, oh)} over the rows of the cases without a cap that plan(W, H, n) lists, for a sink whose windows are on
    the quad grid or not."""
    S = sizes(W, H)
    out = set()
    for name, stops, cap in plan(W, H, n):
        if cap is None and (names is None or any(name.startswith(p) for p in names)):
            for stop in stops:
                ow, oh = S[size_index(W, H, stop)]
                out.add((family(ow, oh, grid_ok), ow, oh))
    return out
