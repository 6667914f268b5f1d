"""Crop decode — test infrastructure only, CPU only: the plan of dwtx_crop_plan (include/dwtx.h) restated, and a numpy
inverse transform that holds nothing but the planned rectangles.

The plan: out[l] is the rectangle of the widths[l] x heights[l] LL band — and, at the same coordinates, of the three detail
bands beside it — that a crop needs; l = levels is the picture, l = 0 the root.  Outputs [a, b) of a line are the pairs
a // 2 .. ceil(b / 2) - 1; icdf53 (cdf53.h:36-61) takes d[k-1] and d[k] for sample 2k and x[2k+2] for sample 2k+1, so the
level below is needed from a // 2 - 1 to ceil(b / 2), clipped to the band.

windowed_inverse() is the check of that claim: it undoes the transform level by level on whole planes, as decode.c:16-30
does, but everything outside the planned rectangles is POISON — in the pyramid before it starts, and in every LL band it
has rebuilt before it goes on.  If the plan kept too little, poison reaches the crop."""
import numpy as np

import orc

POISON = 0x2AAAAAAA55   # far beyond anything 32-bit coefficients add up to: one use of it and no sample can come out right


def plan(W, H, x0, y0, cw, ch):
    """-> [(x0, y0, w, h)] by level, root first"""
    g = orc.geometry(W, H)
    xa, xb, ya, yb = x0, x0 + cw, y0, y0 + ch
    out = [(xa, ya, xb - xa, yb - ya)]
    for l in range(g.levels - 1, -1, -1):
        xa, xb = max(xa // 2 - 1, 0), min((xb + 1) // 2 + 1, g.widths[l])
        ya, yb = max(ya // 2 - 1, 0), min((yb + 1) // 2 + 1, g.heights[l])
        out.append((xa, ya, xb - xa, yb - ya))
    return out[::-1]


def _tdiv(a, n):
    """C's truncating division by 2 or 4 (cdf53.h:13,20 use `/`)"""
    return (a + ((a >> 63) & (n - 1))) // n


def icdf53(s, d, n):
    """cdf53.h:36-61 along axis 0: low half s [ceil(n/2), ...] and high half d [n // 2, ...] -> the n samples"""
    n2 = (n + 1) // 2
    even = s.copy()
    m = n // 2   # the even samples that are updated: all of them, but for the last one of an odd line
    dp = np.concatenate([d[:1], d[:-1]], axis=0)
    even[:m] = s[:m] - _tdiv(dp[:m] + d[:m], 4)
    nxt = np.concatenate([even[1:], even[-1:]], axis=0)   # x[n] := x[n-2]
    odd = d + _tdiv(even[:m] + nxt[:m], 2)
    out = np.empty((n,) + s.shape[1:], dtype=np.int64)
    out[0::2] = even[:n2]
    out[1::2] = odd
    return out


def inverse_level(ll, pyr, w, h):
    """One step of decode.c:16-30: the LL band (h2 x w2) and the detail bands of the w x h corner of the Mallat pyramid ->
    the w x h plane; columns first, then rows (decode.c:21-29)."""
    w2, h2 = (w + 1) // 2, (h + 1) // 2
    p = pyr[:h, :w].astype(np.int64).copy()
    p[:h2, :w2] = ll
    p = icdf53(p[:h2], p[h2:], h)
    return icdf53(p[:, :w2].T, p[:, w2:].T, w).T


def inverse(pyr):
    """The whole inverse of a [H, W] pyramid with inverse_level: held against orc.inverse by tests/test_crop_cpu.py"""
    H, W = pyr.shape
    g = orc.geometry(W, H)
    ll = pyr[:g.heights[0], :g.widths[0]].astype(np.int64)
    for l in range(g.levels):
        ll = inverse_level(ll, pyr, g.widths[l + 1], g.heights[l + 1])
    return ll


def _keep(a, rect):
    """`a` with everything outside the rectangle (clipped to the array) replaced by POISON"""
    x0, y0, w, h = rect
    out = np.full(a.shape, POISON, dtype=np.int64)
    out[y0:y0 + h, x0:x0 + w] = a[y0:y0 + h, x0:x0 + w]
    return out


def windowed_inverse(pyr, x0, y0, cw, ch, rects=None):
    """The cw x ch crop at (x0, y0) of the inverse of the [H, W] pyramid, from the planned rectangles alone."""
    H, W = pyr.shape
    g = orc.geometry(W, H)
    rects = plan(W, H, x0, y0, cw, ch) if rects is None else rects
    held = np.full((H, W), POISON, dtype=np.int64)   # the pyramid with only the planned rectangles of every band
    for l in range(g.levels):
        w, h = g.widths[l + 1], g.heights[l + 1]
        w2, h2 = g.widths[l], g.heights[l]
        for bx, by, bw, bh in ((w2, 0, w - w2, h2), (0, h2, w2, h - h2), (w2, h2, w - w2, h - h2)):
            band = _keep(pyr[by:by + bh, bx:bx + bw].astype(np.int64), rects[l])
            held[by:by + bh, bx:bx + bw] = band
    ll = _keep(pyr[:g.heights[0], :g.widths[0]].astype(np.int64), rects[0])
    for l in range(g.levels):
        ll = _keep(inverse_level(ll, held, g.widths[l + 1], g.heights[l + 1]), rects[l + 1])
    return ll[y0:y0 + ch, x0:x0 + cw]


def sampled_origins(W, H, cw, ch):
    """Origins of a cw x ch crop in a W x H picture: all four parities, all four edges and all four corners."""
    mx, my = W - cw, H - ch
    xs = sorted({0, 1, mx // 2, mx // 2 + 1, mx - 1, mx} & set(range(mx + 1)))
    ys = sorted({0, 1, my // 2, my // 2 + 1, my - 1, my} & set(range(my + 1)))
    return [(x, y) for y in ys for x in xs]
