"""Far layouts — test infrastructure only: the views of tests/test_far_gpu.py, whose windows, planes or rows lie more than
2^31 samples, or 2^32 bytes, from the pointer a call is given, and the host arithmetic that says where everything lies.
Needs no device: tests/test_far_cpu.py checks every claim made here.

A case is a Layout of tests/test_views_gpu.py (a flat buffer of samples, an offset, a shape and strides in samples) plus
the picture's shape, depth and pixel step.  Every address the kernels form for it is a sum of terms, each a product of an
index and a stride: band * band_stride + column * image_stride + channel * channel_stride + y * row_pitch.  `pieces` lists
those terms for every row of every plane of every window.

Two things make a narrow product visible instead of dangerous:
  - HEAD: the view starts 2^31 samples into its frame.  A product that is truncated to a NEGATIVE 32-bit value (a window
    between 2^31 and 2^32 samples out, as `int`) lands before the view, and that is still frame.
  - every far stride is 2^k plus D, a multiple of 4 that is no power of two: a product that wraps modulo 2^32 lands on
    frame between the windows, never on a window and never on a place where the same picture lies.
`stray_rows` forms every such wrong address — each term, and the sum, truncated to 32 bits as a signed and as an unsigned
value, counted in samples and in bytes — and the CPU test asserts that all of them lie inside the frame and outside every
window: a truncated load reads the fill value, a truncated store writes frame that the decode test then finds changed,
and neither leaves the allocation."""
import bisect

from test_views_gpu import Layout

T31, T32 = 1 << 31, 1 << 32
D = 1_000_012        # 4 * 250003: what every far stride has on top of its power of two
HEAD = T31 + 16      # samples of frame in front of the view

WIDE_A, WIDE_B, GENERAL = (132, 68), (68, 260), (131, 68)   # the two smallest wide shapes with a strip edge; the general conversions


def up4(v):
    return (v + 3) // 4 * 4


class Case:
    """L: the Layout; step: the pixel step (0: dense); wide: the lifting kernels read / write the pixels themselves
    (dwtx_pixels_ok), else the general conversions; claims: (s_lo, s_hi, b_lo, b_hi) — some row of the case starts at
    least s_lo and less than s_hi samples, and at least b_lo and less than b_hi bytes, from the view's origin; below: no row
    starts that many samples out or further."""

    def __init__(self, name, wh, Cn, is16, L, wide, claims, step=0, below=None):
        self.name, self.W, self.H, self.Cn, self.is16, self.L, self.wide, self.claims, self.step, self.below = \
            name, wh[0], wh[1], Cn, is16, L, wide, claims, step, below
        self.sb = 2 if is16 else 1

    @property
    def stepped(self):
        return self.step != 0

    @property
    def frame_bytes(self):
        return self.L.samples * self.sb

    def planar(self):
        return self.Cn == 3 and self.L.strides[-2] == 1 and self.L.strides[-1] != 1

    def row_samples(self):
        """from a row's first sample to behind its last (a planar window: of one plane's row)"""
        if self.planar():
            return self.W
        return (self.W - 1) * self.step + self.Cn if self.step else self.W * self.Cn

    def window_terms(self):
        """-> per window [band term, column term], in samples"""
        L = self.L
        if len(L.shape) == 4:
            return [[0, i * L.strides[0]] for i in range(L.shape[0])]
        return [[b * L.strides[0], c * L.strides[1]] for b in range(L.shape[0]) for c in range(L.shape[1])]

    def pieces(self):
        """-> [(terms, length)]: every row of every plane of every window; its terms add up to the row's first sample,
        counted from the view's origin"""
        L = self.L
        planes = [c * L.strides[-1] for c in range(3)] if self.planar() else [0]
        n = self.row_samples()
        return [(wt + [pt, y * L.strides[-3]], n) for wt in self.window_terms() for pt in planes for y in range(self.H)]


INF = 1 << 62
MID = [(T31, T32, 0, INF)]
FAR = [(T32, INF, 0, INF)]
BOTH = MID + FAR


def _stack(wh, Cn, stride, n=3, pad=12, off=0):
    W, H = wh
    pitch = W * Cn + pad
    return Layout(HEAD + off + (n - 1) * stride + H * pitch + 16, HEAD + off, (n, H, W, Cn), (stride, pitch, Cn, 1))


def _grid(wh, Cn, off=0, pad=8):
    """two bands of two windows: the second window of a band just above 2^31 samples from the first, the second band just
    above 2^32 from the first"""
    W, H = wh
    pitch = W * Cn + pad
    istride, bstride = T31 + D, T32 + 3 * D
    return Layout(HEAD + off + bstride + istride + H * pitch + 16, HEAD + off, (2, 2, H, W, Cn), (bstride, istride, pitch, Cn, 1))


def _planar_cs(wh, pad, odd, n=3):
    """the channel planes of the whole view apart (CNHW): stacked windows close together, the G planes just above 2^31
    samples from the R planes, the B planes beyond 2^32"""
    W, H = wh
    pitch = W + pad
    slot = up4(H * pitch + 12)
    cs = T31 + D + odd
    return Layout(HEAD + 2 * cs + n * slot + 16, HEAD, (n, H, W, 3), (slot, pitch, 1, cs))


def _planar_img(wh, pad, off, n=3):
    """planes inside the window (NCHW), the windows just above 2^31 samples apart"""
    W, H = wh
    pitch = W + pad
    cs = up4(H * pitch + 12)
    stride = T31 + D
    return Layout(HEAD + off + (n - 1) * stride + 3 * cs + 16, HEAD + off, (n, H, W, 3), (stride, pitch, 1, cs))


def _rgbx(wh, Cn, off, n=3):
    """4-byte pixels: the RGB of an RGBX8 surface (off 0), or its fourth byte as a gray view (off 3)"""
    W, H = wh
    pitch = 4 * W + 8
    stride = T31 + D
    return Layout(HEAD + (n - 1) * stride + H * pitch + 16, HEAD + off, (n, H, W, Cn), (stride, pitch, 4, 1))


def _far_row(wh, Cn, extra):
    """two windows side by side whose rows are 2^26 + 12 (+ extra) samples apart: y * row_pitch passes 2^31 at row 32 and
    2^32 at row 64 of the 68; the pitch itself fits an int"""
    W, H = wh
    pitch = (1 << 26) + 12 + extra
    istride = 2000
    return Layout(HEAD + (H - 1) * pitch + istride + W * Cn + 16, HEAD, (2, H, W, Cn), (istride, pitch, Cn, 1))


S30 = (1 << 30) + D

CASES = [
    # a stack of three windows, image_stride just above 2^31 samples
    Case("stack-rgb8-wide", WIDE_A, 3, False, _stack(WIDE_A, 3, T31 + D), True, BOTH),
    Case("stack-gray8-general", GENERAL, 1, False, _stack(GENERAL, 1, T31 + D, pad=6, off=1), False, BOTH),
    # five windows just above 2^30 samples apart: enough of them for the decoder to cut the batch into parts
    Case("stack5-rgb8-wide", WIDE_B, 3, False, _stack(WIDE_B, 3, S30, n=5), True, BOTH),
    # a grid, cols = 2, two bands, band_stride just above 2^32
    Case("grid-gray8-wide", WIDE_B, 1, False, _grid(WIDE_B, 1), True, BOTH),
    Case("grid-rgb16-general", GENERAL, 3, True, _grid(GENERAL, 3, off=2, pad=5), False, BOTH),
    # planar RGB, channel_stride just above 2^31: the B plane is past 2^32
    Case("planar-cs-rgb8-wide", WIDE_A, 3, False, _planar_cs(WIDE_A, 8, 0), True, BOTH),
    Case("planar-cs-rgb16-general", GENERAL, 3, True, _planar_cs(GENERAL, 5, 1), False, BOTH),
    # planar RGB, a small channel_stride but a far image_stride
    Case("planar-img-rgb16-wide", WIDE_B, 3, True, _planar_img(WIDE_B, 8, 0), True, BOTH),
    Case("planar-img-rgb8-general", GENERAL, 3, False, _planar_img(GENERAL, 5, 3), False, BOTH),
    # RGBX8 with a far image_stride, and its fourth byte as a gray step-4 view
    Case("rgbx8-rgb-wide", WIDE_A, 3, False, _rgbx(WIDE_A, 3, 0), True, BOTH, step=4),
    Case("rgbx8-alpha-general", WIDE_A, 1, False, _rgbx(WIDE_A, 1, 3), False, BOTH, step=4),
    # a far row: row_pitch 2^26 + 12, H = 68
    Case("far-row-rgb8-wide", WIDE_A, 3, False, _far_row(WIDE_A, 3, 0), True, BOTH),
    Case("far-row-gray8-general", GENERAL, 1, False, _far_row(GENERAL, 1, 1), False, BOTH),
    # 16-bit samples: byte offsets pass 2^31 and 2^32 while every sample offset stays below 2^32 (a byte offset beyond 2^32
    # IS a sample offset beyond 2^31: the second window is the one whose byte offset alone has passed 2^31); and both past 2^32
    Case("stack-gray16-bytes-wide", WIDE_A, 1, True, _stack(WIDE_A, 1, S30), True,
         [(0, T31, T31, T32), (T31, T32, T32, INF)], below=T32),
    Case("stack-rgb16-both-general", GENERAL, 3, True, _stack(GENERAL, 3, T31 + D, pad=5, off=1), False, BOTH),
]
BY_NAME = {c.name: c for c in CASES}
# one group of each kind for the decoder's parts and the rows-per-wave settings: both have four windows or more
SWITCHED = ["stack5-rgb8-wide", "grid-rgb16-general"]


# ---- where a narrow product would land --------------------------------------------------------------------------------

def _s32(v):
    v &= T32 - 1
    return v - T32 if v >= T31 else v


def _u32(v):
    return v & (T32 - 1)


def true_rows(case):
    """-> sorted [(first byte, behind the last byte)] of every row of the case's windows, counted from the frame's start"""
    base = case.L.off * case.sb
    return sorted((base + sum(t) * case.sb, base + (sum(t) + n) * case.sb) for t, n in case.pieces())


def stray_rows(case):
    """-> [(first byte, behind the last byte, what)]: where each row of the case would be read or written if one term of
    its offset, or their sum, were formed in 32 bits — signed or unsigned, in samples or in bytes; only the places that
    differ from the right one"""
    sb, base = case.sb, case.L.off * case.sb
    out = []
    for terms, n in case.pieces():
        right = sum(terms) * sb
        for cut, cname in ((_s32, "int"), (_u32, "unsigned")):
            wrong = []
            for k, t in enumerate(terms):
                rest = (sum(terms) - t) * sb
                wrong.append((rest + cut(t) * sb, f"term {k} as {cname} samples"))
                wrong.append((rest + cut(t * sb), f"term {k} as {cname} bytes"))
            wrong.append((cut(sum(terms)) * sb, f"sum as {cname} samples"))
            wrong.append((cut(right), f"sum as {cname} bytes"))
            out += [(base + o, base + o + n * sb, what) for o, what in wrong if o != right]
    return out


def overlaps(rows, a, b):
    """does [a, b) meet one of the sorted, disjoint intervals `rows`?"""
    k = bisect.bisect_right(rows, (a, 1 << 62))
    return (k > 0 and rows[k - 1][1] > a) or (k < len(rows) and rows[k][0] < b)


# ---- what the library asks of a view (include/dwtx.h, dwtx_internal.h), restated ----------------------------------------

def decode_view_accepts(case):
    """The disjointness rules of dwtx_decode_view / dwtx_decode_view_step as include/dwtx.h states them -> None, or the
    rule that fails."""
    import dwt_amd

    f = dwt_amd.view_fields(case.L.shape, case.L.strides, case.stepped)
    W, H, n = f["W"], f["H"], f["n"]
    cols = min(f["cols"] or n, n)
    pitch, istride, bstride, cs = f["row_pitch"], f["image_stride"], f["band_stride"], f["channel_stride"]
    row = case.row_samples()
    if pitch < row:
        return "row_pitch below a row"
    window = (H - 1) * pitch + row
    nbands = -(-n // cols)
    stacked = istride >= window
    beside = istride >= row and pitch >= (cols - 1) * istride + row
    if cs:
        win3 = 2 * cs + window
        if cs >= window and (cols == 1 or istride >= win3) and (nbands == 1 or bstride >= (cols - 1) * istride + win3):
            return None
    if cols > 1 and not stacked and not beside:
        return "windows overlap"
    if nbands > 1 and bstride < (cols - 1) * istride + window:
        return "bands overlap"
    if cs and cs < (nbands - 1) * bstride + (cols - 1) * istride + window:
        return "planes overlap"
    return None


def wide_conditions(case):
    """dwtx_pixels_ok (lift.hip) for the case, given a frame that starts on a 16-byte boundary: W % 4 == 0, a side above
    64, dwtx_pixels::wide() — every stride and the origin on the quad grid —, a pitch that fits an int, and of the stepped
    views only 8-bit RGB in 4-byte pixels."""
    import dwt_amd

    f = dwt_amd.view_fields(case.L.shape, case.L.strides, case.stepped)
    quad = all(f[k] % 4 == 0 for k in ("row_pitch", "image_stride", "band_stride", "channel_stride")) and case.L.off % 4 == 0
    rgbx8 = f["pixel_step"] == 4 and case.Cn == 3 and not case.is16
    return case.W % 4 == 0 and (case.W > 64 or case.H > 64) and quad and f["row_pitch"] < T31 and (not f["pixel_step"] or rgbx8)
