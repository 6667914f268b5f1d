"""Crop decode — test infrastructure only, CPU only: the plan of dwtx_crop_plan (include/dwtx.h) restated, and a numpy
inverse transform that holds nothing but the planned rectangles.

The plan: out[l] is the rectangle of the widths[l] x heights[l] LL band — and, at the same coordinates, of the three detail
bands beside it — that a crop needs; l = levels is the picture, l = 0 the root.  Outputs [a, b) of a line are the pairs
a // 2 .. ceil(b / 2) - 1; icdf53 (cdf53.h:36-61) takes d[k-1] and d[k] for sample 2k and x[2k+2] for sample 2k+1, so the
level below is needed from a // 2 - 1 to ceil(b / 2), clipped to the band.

windowed_inverse() is the check of that claim: it undoes the transform level by level on whole planes, as decode.c:16-30
does, but everything outside the planned rectangles is POISON — in the pyramid before it starts, and in every LL band it
has rebuilt before it goes on.  If the plan kept too little, poison reaches the crop.

The kernel path (dwtx_inv_crop) has rectangles of its own — one size per plane for all pictures of a launch, origins per
picture: kernel_steps(), kernel_origins() and kernel_reads() restate them and what k_inv_level_roi fetches, and
sweep_groups() lists the cases of tests/test_crop_sweep_gpu.py, which tests/test_crop_sweep_cpu.py holds against them."""
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


# ---- the kernel path's rectangles (dwtx_inv_crop, lift.hip section "crop decode") -----------------------------------------
# dwtx_decode_view_crop does not go through dwtx_crop_plan: all pictures of a launch share one rectangle size per plane
# (dwtx_crop_steps_of) and every picture has origins of its own (dwtx_crop_origins).  Planes are counted as lift.hip counts
# them: t = 0 is the picture, t = T the root.

TAIL_MAX = 64      # lift.hip: constexpr int TAIL_MAX — no side above it: the rest of the transform is one LDS launch
MIN_LEN = 8        # include/dwtx.h: DWTX_MIN_LEN
MAX_LEVELS = 16    # include/dwtx.h: DWTX_MAX_LEVELS
INV_PAIRS = 62     # lift.hip: constexpr int INV_PAIRS — pairs a workgroup's 64 lanes write (one halo lane on each side)


class Steps:
    """dwtx_crop_steps (dwtx_internal.h): T, tail_from; ws, hs: the whole planes 0 .. T; w, h: the rectangles' sizes"""

    def __init__(self, T, tail_from, ws, hs, w, h):
        self.T, self.tail_from, self.ws, self.hs, self.w, self.h = T, tail_from, ws, hs, w, h


def kernel_steps(W, H, cw, ch):
    """lift_layout (lift.hip: `do { ws[n + 1] = (ws[n] + 1) >> 1 ... } while (n < DWTX_MAX_LEVELS && ws[n] >= DWTX_MIN_LEN &&
    hs[n] >= DWTX_MIN_LEN)`, `while (t < n && (ws[t] > TAIL_MAX || hs[t] > TAIL_MAX)) ++t`) and dwtx_crop_steps_of
    (`S->w[t] = t == 0 ? cw : whole ? L.ws[t] : min(L.ws[t], S->w[t - 1] / 2 + 3)` with `whole = t >= L.tail_from`)."""
    assert 1 <= cw <= W and 1 <= ch <= H
    ws, hs, n = [W], [H], 0
    while True:
        ws.append((ws[n] + 1) >> 1)
        hs.append((hs[n] + 1) >> 1)
        n += 1
        if not (n < MAX_LEVELS and ws[n] >= MIN_LEN and hs[n] >= MIN_LEN):
            break
    T, t = n, 0
    while t < n and (ws[t] > TAIL_MAX or hs[t] > TAIL_MAX):
        t += 1
    tail_from = t
    w, h = [cw], [ch]
    for t in range(1, T + 1):
        whole = t >= tail_from
        w.append(ws[t] if whole else min(ws[t], w[t - 1] // 2 + 3))
        h.append(hs[t] if whole else min(hs[t], h[t - 1] // 2 + 3))
    return Steps(T, tail_from, ws, hs, w, h)


def kernel_origins(S, x0, y0):
    """dwtx_crop_origins: `xs[t] = max(0, min((xs[t - 1] >> 1) - 1, S.ws[t] - S.w[t]))` -> (xs, ys), planes 0 .. T"""
    xs, ys = [x0], [y0]   # (integers, or numpy arrays of them: many origins at once)
    for t in range(1, S.T + 1):
        xs.append(np.maximum(0, np.minimum((xs[t - 1] >> 1) - 1, S.ws[t] - S.w[t])))
        ys.append(np.maximum(0, np.minimum((ys[t - 1] >> 1) - 1, S.hs[t] - S.h[t])))
    return xs, ys


def pair_range(d0, dn):
    """k_inv_level_roi: `kA = dx >> 1, kB = (dx + a.dw + 1) >> 1` — the pairs kA .. kB - 1 hold samples d0 .. d0 + dn - 1"""
    return d0 >> 1, (d0 + dn + 1) >> 1


def kernel_reads(S, xs, ys, t):
    """The LL samples of plane t + 1 that the launch of step t (k_inv_level_roi, t < tail_from) fetches for one picture
    -> (k_lo, k_hi, j_lo, j_hi), inclusive, in the whole plane's coordinates.
    Columns: a strip's lanes hold the pairs kb - 1 + lane from kb = kA + 62 * blockIdx.x on, and fetch where `mine = L.k >= 0
    && L.k <= kB` and `2 * L.k < a.w`: the pairs max(kA - 1, 0) .. min(kB, w2 - 1), for every strip together.  (Pair kA - 1
    is fetched, but only its detail half is used.)
    Rows: a wave strip fetches LL row j0 (`fetch(j0, ...)`) and then row jj + 1 for jj < j1 <= jB where `r1 + 1 < a.h`, that
    is jj + 1 < h2; row pair j0 - 1 is read from the detail bands alone (`details(j0 - 1, ...)`), which lie whole in the
    pyramid.  All wave strips together: jA .. min(jB, h2 - 1)."""
    assert 0 <= t < S.tail_from
    kA, kB = pair_range(xs[t], S.w[t])
    jA, jB = pair_range(ys[t], S.h[t])
    return np.maximum(kA - 1, 0), np.minimum(kB, S.ws[t + 1] - 1), jA, np.minimum(jB, S.hs[t + 1] - 1)


def kernel_rects(S, xs, ys):
    """The kernel path's rectangles in plan()'s form, root first, as windowed_inverse(rects=) takes them.  (That function keeps
    the same rectangle of the detail bands too, which the kernel reads whole: it asks for more than the kernel needs.)"""
    return [(xs[t], ys[t], S.w[t], S.h[t]) for t in range(S.T, -1, -1)]


def launch_strips(S, xs, ys, t, rows_per_wave):
    """-> (62-pair strips, wave strips of rows_per_wave row pairs) of step t's launch that hold samples of this picture's
    rectangle: the workgroups and waves that do not leave at `if (kb >= kB || j0 >= jB) return`"""
    kA, kB = pair_range(xs[t], S.w[t])
    jA, jB = pair_range(ys[t], S.h[t])
    return -(-(kB - kA) // INV_PAIRS), -(-(jB - jA) // rows_per_wave)


def classes(S, xs, ys, t, rows_per_wave=0):
    """What one picture's rectangle of plane t (t < tail_from: the destination of step t, and for t >= 1 the source of step
    t - 1) is, per axis -> {(axis, word)}:
    even / odd: the origin's parity; at0 / far / free: (t >= 1, rectangles narrower than their band) whether dwtx_crop_origins
    moved the origin up to 0, back from the far edge, or left it at (previous >> 1) - 1; narrow / band: narrower than the
    plane or all of it; frozen / thawed: whether it holds the last sample of an odd line, which icdf53 leaves as it is;
    strips1 / strips2: (x) one, or at least two, 62-pair strips; waves2: (y, under a forced rows_per_wave) at least two wave
    strips."""
    out = set()
    strips = launch_strips(S, xs, ys, t, rows_per_wave or 1)
    for axis, o, n, N, count in (("x", xs, S.w, S.ws, strips[0]), ("y", ys, S.h, S.hs, strips[1])):
        out.add((axis, "odd" if o[t] & 1 else "even"))
        out.add((axis, "narrow" if n[t] < N[t] else "band"))
        if t >= 1 and n[t] < N[t]:
            a, far = (o[t - 1] >> 1) - 1, N[t] - n[t]
            out.add((axis, "at0" if a < 0 else "far" if a > far else "free"))
        out.add((axis, "frozen" if (N[t] & 1) and o[t] + n[t] == N[t] else "thawed"))
        if axis == "x":
            out.add((axis, "strips1" if count == 1 else "strips2"))
        elif rows_per_wave and count >= 2:
            out.add((axis, "waves2"))
    return out


# ---- the sweep: the cases of tests/test_crop_sweep_gpu.py, kept here so that tests/test_crop_sweep_cpu.py can say what they reach --

CALL_MAX = 512     # pictures per call: four decoder parts, each with its own slice of the origin table
GROUP_MAX = 4096   # origins per test id


class Case:
    """One crop size of one shape at a list of origins: one call, or one per CALL_MAX origins.  route: DWTX_OPT_CROP_ROUTE;
    rows_per_wave: DWTX_OPT_LIFT_ROWS; reduced: (W, H) of the streams, which stop one level early and give a W x H picture —
    the origins may then lie across its edges and beyond them."""

    def __init__(self, W, H, Cn, cw, ch, origins, route=1, rows_per_wave=0, reduced=None):
        self.W, self.H, self.Cn, self.cw, self.ch, self.origins = W, H, Cn, cw, ch, list(origins)
        self.route, self.rows_per_wave, self.reduced = route, rows_per_wave, reduced

    def launches(self):
        """-> [(Steps, origins)]: what dwtx_inv_crop is called with.  Whole pictures: one size for all origins; reduced ones
        come one by one with the part of the crop that lies inside the picture (codec.hip, `finish`), if any."""
        if not self.reduced:
            return [(kernel_steps(self.W, self.H, self.cw, self.ch), self.origins)]
        out = []
        for x0, y0 in self.origins:
            cw, ch = min(x0 + self.cw, self.W) - x0, min(y0 + self.ch, self.H) - y0
            if cw >= 1 and ch >= 1:
                out.append((kernel_steps(self.W, self.H, cw, ch), [(x0, y0)]))
        return out


def every_origin(W, H, cw, ch, ys=None):
    return [(x, y) for y in (range(H - ch + 1) if ys is None else ys) for x in range(W - cw + 1)]


def corners(W, H):
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]


THIN = [(300, 9), (9, 300), (65, 8), (8, 65), (40, 200), (200, 40), (300, 17), (17, 300)]
THIN_RGB = [(300, 9), (40, 200)]
REDUCED = (266, 266, 133, 133)   # streams of 266 x 266 that stop one level early: pictures of 133 x 133


def sweep_groups():
    """-> {test id: [Case]}, in the order of the issue's lists: every origin, strip edges, every size, thin shapes, a shape
    with three windowed levels, reduced pictures."""
    G = {}

    def add(name, W, H, Cn, cw, ch, origins, **kw):
        origins = list(origins)
        parts = [origins[i:i + GROUP_MAX] for i in range(0, len(origins), GROUP_MAX)]
        for p, part in enumerate(parts):
            key = name if len(parts) == 1 else "%s-part%d" % (name, p)
            G.setdefault(key, []).append(Case(W, H, Cn, cw, ch, part, **kw))

    # every origin: 133 -> 67 -> 34, both windowed planes odd; 136 -> 68 -> 34 and 132 -> 66 -> 33, both even; 70 x 67 RGB, one
    # windowed level, the origin table indexed by plane / 3, under every route
    add("every-133x133-gray-9x7", 133, 133, 1, 9, 7, every_origin(133, 133, 9, 7))
    add("every-136x132-gray-10x8", 136, 132, 1, 10, 8, every_origin(136, 132, 10, 8))
    for route in (1, 0, 2):
        add("every-70x67-rgb-9x7-route%d" % route, 70, 67, 3, 9, 7, every_origin(70, 67, 9, 7), route=route)
    # DWTX_OPT_LIFT_ROWS 4: a 23-row crop lies in 12 or 13 row pairs, three or four wave strips, and its 14 rows of plane 1 in two
    add("every-133x133-gray-9x23-rows4", 133, 133, 1, 9, 23, every_origin(133, 133, 9, 23), rows_per_wave=4)
    # strip edges: 250 columns are three 62-pair strips of plane 0 and two of plane 1, starting at every kA; 124 and 126 columns
    # are the sizes on either side of the step from one strip to two
    add("strips-300x72-gray-250x11", 300, 72, 1, 250, 11, every_origin(300, 72, 250, 11))
    for cw in (124, 126):
        add("strips-300x72-gray-%dx11" % cw, 300, 72, 1, cw, 11, every_origin(300, 72, cw, 11, ys=(0, 1, 61)))
    # every size at the sampled origins: pairs_x = dw / 2 + 1 and min(ws, w / 2 + 3) through every value up to the whole band
    for cw in range(1, 134):
        add("sizes-133x133-gray-cw", 133, 133, 1, cw, 7, sampled_origins(133, 133, cw, 7))
    for ch in range(1, 134):
        add("sizes-133x133-gray-ch", 133, 133, 1, 9, ch, sampled_origins(133, 133, 9, ch))
    for cw in range(1, 301):
        add("sizes-300x72-gray-cw%s" % ("-to150" if cw <= 150 else "-from151"), 300, 72, 1, cw, 11, sampled_origins(300, 72, cw, 11))
    # thin shapes: every origin of a 7 x 5 crop, the four 1 x 1 corners, the crops one short of the whole picture
    for W, H in THIN:
        for Cn in (1, 3) if (W, H) in THIN_RGB else (1,):
            name = "thin-%dx%d-%s" % (W, H, "rgb" if Cn == 3 else "gray")
            cw, ch = min(7, W), min(5, H)
            add(name + "-%dx%d" % (cw, ch), W, H, Cn, cw, ch, every_origin(W, H, cw, ch))
            add(name + "-edges", W, H, Cn, 1, 1, corners(W, H))
            add(name + "-edges", W, H, Cn, W - 1, H, [(0, 0), (1, 0)])
            add(name + "-edges", W, H, Cn, W, H - 1, [(0, 0), (0, 1)])
            add(name + "-edges", W, H, Cn, W - 1, H - 1, [(0, 0), (1, 0), (0, 1), (1, 1)])
    # three windowed levels whose third plane is odd on both axes (299 -> 150 -> 75 -> 38, 291 -> 146 -> 73 -> 37): a small crop,
    # and one large enough that its rectangle of plane 2 is the whole band
    for cw, ch in ((9, 7), (290, 283)):
        add("deep-299x291-gray", 299, 291, 1, cw, ch, sampled_origins(299, 291, cw, ch))
    # reduced pictures, launched one by one with scalar origins: inside, across the right and bottom edges, beyond them
    W, H, ow, oh = REDUCED
    across = [(ow - 4, 60), (60, oh - 3), (ow - 1, oh - 1), (ow - 8, oh - 6)]
    beyond = [(ow, 60), (60, oh), (ow + 7, oh + 7), (W - 9, H - 7)]
    add("reduced-266x266-gray-9x7", ow, oh, 1, 9, 7, sampled_origins(ow, oh, 9, 7) + across + beyond, reduced=(W, H))
    return G


_sweep_streams = {}


def sweep_stream(case):
    """-> (the .dwt of the case's picture, the oracle's decode of it): one noise picture per shape (orc.synth kind 1: every
    sample a hash of its position), encoded and decoded by the oracle once.
    Reduced pictures: a stream of plain noise that stops early has lost the low bit planes of every level, and what it gives
    is smooth in places.  So the picture is noise one level down — a noise picture of the reduced size as the LL band of a
    pyramid whose finest detail bands are zero, inverted: 64 .. 191, no clamp — and its stream is cut one byte short of the
    finest level (levels.late_prefix)."""
    import levels

    W, H = case.reduced or (case.W, case.H)
    key = (W, H, case.Cn, case.reduced is not None)
    if key not in _sweep_streams:
        seed = 7000 + W + H + case.Cn
        if case.reduced:
            pyr = np.zeros((H, W, case.Cn), dtype=np.int32)
            pyr[:case.H, :case.W] = orc.forward(orc.synth(case.W, case.H, case.Cn, seed, 1).astype(np.int32) // 2 + 64)
            pic = orc.inverse(pyr)
            assert pic.min() >= 0 and pic.max() <= 255
            data = orc.encode(pic.astype(np.uint8))[0]
            data = levels.late_prefix(data, W, H, case.Cn, levels.levels_of(W, H) - 2)
        else:
            data = orc.encode(orc.synth(W, H, case.Cn, seed, 1))[0]
        pic = orc.decode(data)
        assert pic.shape == (case.H, case.W, case.Cn)
        pic.setflags(write=False)
        _sweep_streams[key] = (data, pic)
    return _sweep_streams[key]
