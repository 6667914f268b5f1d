"""Deep pixels (samples of more than 8 bits) on the CPU — test infrastructure only.

The reference reads 8-bit PNM and nothing else, but its algorithm does not know the depth: encode.c:155-221 and
decode.c:174-264 work on `int`.  What it would write for wider samples is therefore the composition of the oracle's
depth-agnostic stages, each of which is pinned on the reference by tests/test_oracle.py:

    deep_encode = orc.forward -> orc.linearize -> orc.encode_lin      (after YCoCg-R for colour, image.h:53-65)
    deep_decode = orc.decode_stage -> orc.reconstruct -> orc.inverse  (then image.h:39-51 and pnm.h:108 with the
                                                                       picture's maxval where those have 255)

tests/test_deep_cpu.py checks that the composition equals the whole-file oracle (orc.encode / orc.decode) on 8-bit
pictures and the reference binary's own bytes (tests/golden/smpte*.dwt).

Also here: seeded integer-only generators of deep pictures, the pictures, streams and batches of
tests/test_foreign_depth_gpu.py (deep streams through the 8-bit decoders) with the conditions its inputs must meet, and
the linear gain model of the transform that says which depths can never need more than the coder's 16 bit planes
(DESIGN.md section 4.8)."""
import numpy as np

import orc


def tdiv2(x):
    """C's truncating /2."""
    return np.where(x < 0, -((-x) // 2), x // 2)


def rgb2ycocg(p):
    """image.h:53-65."""
    p = p.astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    U = R - B
    T = B + tdiv2(U)
    V = G - T
    Y = T + tdiv2(V)
    return np.stack([Y, U, V], -1).astype(np.int32)


def ycocg2rgb(p, M=None):
    """image.h:39-51 with M where it has 255, then pnm.h:108's clamp; M = None: the arithmetic without any clamp."""
    p = p.astype(np.int64)
    Y, U, V = p[..., 0], p[..., 1], p[..., 2]
    if M is not None:
        Y, U, V = np.clip(Y, 0, M), np.clip(U, -M, M), np.clip(V, -M, M)
    T = Y - tdiv2(V)
    G = V + T
    B = T - tdiv2(U)
    R = B + U
    out = np.stack([R, G, B], -1)
    return out if M is None else np.clip(out, 0, M)


def deep_encode(pix, capacity=0):
    """integer pixels [H, W, C] of any depth -> (.dwt bytes, orc.Stats)."""
    H, W, C = pix.shape
    a = rgb2ycocg(pix) if C == 3 else pix.astype(np.int32)
    return orc.encode_lin(orc.linearize(orc.forward(a)), W, H, capacity)


def decoded(data, W, H, C, pixels_max=-1):
    """.dwt bytes (or a prefix) -> (level, missing, plane counts, int32 [h, w, C]: the inverse transform's output before the
    colour transform and every clamp — Y, Co, Cg for C == 3), or None where decode.c would exit 1."""
    r = orc.decode_stage(data, W, H, C, pixels_max)
    if r is None:
        return None
    lin, level, missing, planes = r
    return level, missing, planes, orc.inverse(orc.reconstruct(lin, W, H, level + 1, missing))


def to_pixels(img, C, M):
    """image.h:39-51 and pnm.h:108 with M where they have 255 on the inverse transform's output -> uint16 [h, w, C]."""
    return (ycocg2rgb(img, M) if C == 3 else np.clip(img, 0, M)).astype(np.uint16)


def deep_decode(data, W, H, C, M, pixels_max=-1, clamp=True):
    """.dwt bytes (or a prefix) -> uint16 [h, w, C] with the clamps at M, or None where decode.c would exit 1.
    clamp=False: int64 samples as the arithmetic leaves them, no clamp anywhere."""
    r = decoded(data, W, H, C, pixels_max)
    if r is None:
        return None
    img = r[3]
    if not clamp:
        return ycocg2rgb(img, None) if C == 3 else img.astype(np.int64)
    return to_pixels(img, C, M)


def levels_max(W, H, pixels_max):
    """decode.c:165-171: the PIXELS argument as the level cap the device entry points take."""
    if pixels_max < 0:
        return -1
    g = orc.geometry(W, H)
    lm = g.levels
    while lm > 0 and g.pixels[lm] > pixels_max:
        lm -= 1
    return lm


# ---- pictures (numpy, integer only, seeded) --------------------------------------------------------------------

def smooth_noise(W, H, C, M, seed=0):
    """Triangle ramps (periods 192 and 128, as orc.synth's) scaled to 7/8 of M, M/64 per channel, M/32 of noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    ramp = (np.abs(x % 192 - 96) + np.abs(y % 128 - 64)).astype(np.int64) * (M * 7 // 8) // 160
    k = np.arange(C, dtype=np.int64) * (M // 64)
    noise = rng.integers(0, M // 32 + 1, (H, W, C), dtype=np.int64)
    return (ramp[..., None] + k + noise).astype(np.uint16)


def noise(W, H, C, M, seed=0):
    return np.random.default_rng(seed).integers(0, M + 1, (H, W, C), dtype=np.int64).astype(np.uint16)


def checker(W, H, C, M):
    """Alternating 0 / M; of three channels the middle one is inverted."""
    y, x = np.mgrid[:H, :W]
    c = (((x + y) & 1) * M).astype(np.uint16)
    p = np.repeat(c[..., None], C, axis=2)
    if C == 3:
        p[..., 1] = M - c
    return p


def blocks(W, H, C, M, seed=0):
    """3x5-pixel (rows x columns) blocks of 0 / M, every channel its own."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, ((H + 2) // 3, (W + 4) // 5, C), dtype=np.int64)
    return (np.repeat(np.repeat(bits, 3, axis=0), 5, axis=1)[:H, :W] * M).astype(np.uint16)


def impulses(W, H, C, V, seed, base=511, share=0.004):
    """Uniform noise in [0, base] with a `share` of the pixels set to V (of three channels R and B get V and G gets 0,
    so that Cg carries the impulse as well as Y).  The isolated samples make coefficients of about 2 * V on the finest
    levels, so V picks the plane count, while most of the picture stays small: an 8-bit decode of such a stream has
    about half of its samples inside [0, 255] and the rest cut by every clamp.  (Plain deep noise saturates nearly
    everywhere.)"""
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, base + 1, (H, W, C), dtype=np.int64)
    at = rng.choice(W * H, max(1, round(share * W * H)), replace=False)
    flat = pix.reshape(W * H, C)
    flat[at] = (V, 0, V) if C == 3 else (V,)
    return pix.astype(np.uint16)


# The pictures of tests/test_foreign_depth_gpu.py: impulses(W, H, C, V, FOREIGN_SEED) with, per (W, H, C), the largest V
# that needs 15 bit planes — its largest coefficient is then 32767 in magnitude, the last value an int16 holds — and that
# V + 6000, which needs 16.  tests/test_deep_cpu.py holds every one of them to what the GPU tests rely on.
FOREIGN_SEED = 3
FOREIGN_WIDE = [(132, 72), (516, 260), (1088, 320)]   # W, H: the fused inverse kernels; 1088x320 has five 16-bit ring levels
FOREIGN_GENERAL = [(131, 77), (64, 48)]               # W % 4 != 0; nothing above the LDS tail
FOREIGN_V = {(132, 72, 1): 32678, (132, 72, 3): 32217, (516, 260, 1): 26482, (516, 260, 3): 26310, (1088, 320, 1): 26384,
             (1088, 320, 3): 26029, (131, 77, 1): 32714, (131, 77, 3): 32650, (64, 48, 1): 33067, (64, 48, 3): 32779}
_foreign = {}


def foreign_picture(W, H, C, planes, seed=FOREIGN_SEED):
    """The 15- or 16-plane picture of a geometry; another seed: 15 planes with room to spare (V = 24000), or 16."""
    if seed == FOREIGN_SEED:
        return impulses(W, H, C, FOREIGN_V[W, H, C] + (6000 if planes == 16 else 0), seed)
    return impulses(W, H, C, 24000 if planes == 15 else 40000, seed)


def foreign_stream(W, H, C, planes, seed=FOREIGN_SEED):
    """-> (.dwt bytes, Stats) of foreign_picture, made once."""
    key = (W, H, C, planes, seed)
    if key not in _foreign:
        _foreign[key] = deep_encode(foreign_picture(W, H, C, planes, seed))
    return _foreign[key]


def foreign_cuts(data):
    """The two prefixes that still reach the finest level (tests/test_deep_cpu.py), so that the dequantisation bias of
    decode.c:32-65 is added to coefficients of every size."""
    return [data[:len(data) * 3 // 4], data[:len(data) // 2]]


def level_early_cut(data, W, H, C):
    """The longest prefix whose decode stops one level short of the whole picture (or earlier)."""
    key = (data, "early")
    if key not in _foreign:
        levels = orc.geometry(W, H).levels
        lo, hi = 6, len(data)   # (6 bytes are unreadable; the whole stream reaches the last level)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            r = orc.decode_stage(data[:mid], W, H, C)
            if r is None or r[1] < levels - 1:
                lo = mid
            else:
                hi = mid
        _foreign[key] = data[:lo]
    return _foreign[key]


REFUSED = "17 planes"   # the name of the row every decoder must answer with status 2


def foreign_rows(W, H, C):
    """[(name, .dwt bytes)]: what no 8-bit picture makes — whole 15- and 16-plane streams, their cuts — beside what one
    does, and a stream that claims 17 planes."""
    s15, s16 = foreign_stream(W, H, C, 15)[0], foreign_stream(W, H, C, 16)[0]
    c15, c16 = foreign_cuts(s15), foreign_cuts(s16)
    return [("15 planes", s15), ("16 planes", s16), ("15 planes, 3/4", c15[0]), ("16 planes, 3/4", c16[0]),
            ("15 planes, 1/2", c15[1]), ("16 planes, 1/2", c16[1]), ("15 planes, a level early", level_early_cut(s15, W, H, C)),
            ("8-bit picture", orc.encode(orc.synth(W, H, C, 7, 0))[0]), (REFUSED, orc.many_plane_stream(W, H, C, [17, 3, 3]))]


def foreign_clean_rows(W, H, C):
    """Six rows that every decoder part takes whole and with at most 15 planes, so that the 16-bit ring planes carry
    them wherever the shape has any: the stream that reaches 32767, its two cuts, an 8-bit picture's and two more seeds."""
    s15 = foreign_stream(W, H, C, 15)[0]
    c15 = foreign_cuts(s15)
    return [("15 planes", s15), ("15 planes, 3/4", c15[0]), ("15 planes, 1/2", c15[1]), ("8-bit picture", orc.encode(orc.synth(W, H, C, 7, 0))[0]),
            ("15 planes, seed 11", foreign_stream(W, H, C, 15, 11)[0]), ("15 planes, seed 12", foreign_stream(W, H, C, 15, 12)[0])]


def decoder_parts(n, K=0):
    """The ranges of rows dwtx_decode_planes_ex cuts a batch of n into under DWTX_OPT_DECODE_PARTS = K (0: automatic;
    K = 1 stands for DWTX_OPT_ONE_STREAM): unpack.hip, "Parts"."""
    if n < 4 or K == 1:
        K = 1
    elif K == 0:
        K = 4 if n >= 24 else 2
    K = min(max(K, 1), 4)
    return [range(n * k // K, n * (k + 1) // K) for k in range(K)]


def clean_parts(rows, W, H, C, K=0):
    """The parts of a batch (decoder_parts) that scatter() of unpack.hip sends through the 16-bit ring planes: every row
    readable, decoded to the last level, and none with more than 15 planes."""
    levels = orc.geometry(W, H).levels

    def clean(row):
        key = (row[1], "clean")
        if key not in _foreign:
            r = None if row[0] == REFUSED else orc.decode_stage(row[1], W, H, C)
            _foreign[key] = r is not None and r[1] == levels - 1 and max(r[3]) <= 15
        return _foreign[key]
    flags = [clean(row) for row in rows]
    return [p for p in decoder_parts(len(rows), K) if all(flags[i] for i in p)]


def levels16(W, H):
    """The mask of ring levels that dwtx_transformation_fwd_pixels reports as 16-bit for a W x H picture (lift.hip,
    dwtx_levels16 over linearize.hip's dwtx_square_levels), restated: from the finest level down, at most five, while
    the step is above the 64 x 64 LDS tail, its width a multiple of 4 and the level's Hilbert square at least 64 wide.
    tests/test_foreign_depth_gpu.py compares it with what the library reports."""
    g = orc.geometry(W, H)
    if W % 4:
        return 0
    mask, w, h = 0, W, H
    for t in range(min(5, g.levels)):
        l = g.levels - 1 - t
        if (w <= 64 and h <= 64) or w % 4 or g.lengths[l + 1] < 64:
            break
        mask |= 1 << l
        w, h = (w + 1) >> 1, (h + 1) >> 1
    return mask


def ring_level_tops(pic):
    """The largest |coefficient| of a picture on every ring level, finest last (the oracle's linearised planes)."""
    H, W, C = pic.shape
    g = orc.geometry(W, H)
    lin = np.abs(orc.linearize(orc.forward(rgb2ycocg(pic) if C == 3 else pic.astype(np.int32))))
    return [int(lin[:, g.pixels[l]:g.pixels[l + 1]].max()) for l in range(g.levels)]


FOREIGN_BATCH_16 = 5   # where the 16-plane stream of foreign_batch stands


def foreign_batch(W, H, C):
    """Twelve rows around one 16-plane stream.  The decoder cuts a batch of n into K parts [n*k/K, n*(k+1)/K) and asks
    of each part whether any of its streams has more than 15 planes: at index 5 the 16-plane stream shares a part with
    rows 0-4 (K = 2), with 4, 6 and 7 (K = 3), with 3 and 4 (K = 4) and with all (K = 1).  The refused row stands in the
    first part of every K, so the rows from 6 on (K = 2), 8 on (K = 3) and 6 on (K = 4) are parts of whole streams of at most
    15 planes, which take the 16-bit planes beside the part that may not; the stream whose coefficients reach 32767 is
    row 9, in such a part for every K above 1 (clean_parts; tests/test_deep_cpu.py)."""
    w15 = lambda seed: foreign_stream(W, H, C, 15, seed)[0]   # noqa: E731
    s15, s16 = foreign_stream(W, H, C, 15)[0], foreign_stream(W, H, C, 16)[0]
    rows = [("15 planes, seed 11", w15(11)), ("8-bit picture", orc.encode(orc.synth(W, H, C, 8, 1))[0]), (REFUSED, orc.many_plane_stream(W, H, C, [17, 3, 3])),
            ("15 planes, seed 14", w15(14)), ("15 planes, seed 12", w15(12)), ("16 planes", s16), ("15 planes, seed 13", w15(13)),
            ("8-bit picture", orc.encode(orc.synth(W, H, C, 9, 0))[0]), ("15 planes, 1/2", foreign_cuts(s15)[1]), ("15 planes", s15),
            ("15 planes, 3/4", foreign_cuts(s15)[0]), ("15 planes, seed 15", w15(15))]
    assert rows[FOREIGN_BATCH_16][0] == "16 planes"
    return rows


FOREIGN_BATCH_SHAPES = [(132, 72, 1), (132, 72, 3), (516, 260, 3), (1088, 320, 3)]   # W, H, C of the batches
FOREIGN_SEEDS = (FOREIGN_SEED, 11, 12, 13, 14, 15)


def foreign_uniform(W, H, C, planes):
    """Six whole streams that all need `planes` bit planes."""
    return [("%d planes, seed %d" % (planes, s), foreign_stream(W, H, C, planes, s)[0]) for s in FOREIGN_SEEDS]


def clamp_shares(img, C):
    """What the clamps of image.h:39-51 / pnm.h:108 at 255 find in an inverse transform's output [..., C] (int, before
    any clamp): (share of the final samples inside [0, 255], [share of Y outside [0, 255], of Co and of Cg outside
    [-255, 255]]) — the list is empty for gray."""
    a = img.astype(np.int64)
    if C == 1:
        return float(((a >= 0) & (a <= 255)).mean()), []
    out = ycocg2rgb(a, None)
    return (float(((out >= 0) & (out <= 255)).mean()),
            [float(((a[..., 0] < 0) | (a[..., 0] > 255)).mean())] + [float((np.abs(a[..., c]) > 255).mean()) for c in (1, 2)])


def clamps_are_at_work(img, C):
    """The condition every 8-bit clamp test here asserts of its input: between 25 % and 75 % of the samples end inside
    [0, 255], and each of Y, Co and Cg leaves its clamp on 10 % to 90 % of the samples."""
    inside, outside = clamp_shares(img, C)
    return 0.25 <= inside <= 0.75 and all(0.10 <= s <= 0.90 for s in outside)


# ---- the transform's gain ----------------------------------------------------------------------------------------

def _step(X):
    """One level of cdf53.h:9-34 without the roundings, on the rows of X (row = sample): its first / last-sample rules
    and the evens-then-odds order."""
    X = X.copy()
    N = X.shape[0]
    odd = np.arange(1, N - 1, 2)
    X[odd] -= (X[odd - 1] + X[odd + 1]) / 2          # cdf53.h:12-14
    if N % 2 == 0:
        X[N - 1] -= X[N - 2]                         # cdf53.h:15-17
    X[0] += X[1] / 2                                 # cdf53.h:19-20
    ev = np.arange(2, N & ~1, 2)
    X[ev] += (X[ev - 1] + X[ev + 1]) / 4             # cdf53.h:21-23
    return np.concatenate([X[0::2], X[1::2]])        # cdf53.h:25-33


class Gain:
    """gray, chroma: the largest |coefficient| / maxval any detail coefficient of a W x H picture can reach, for
    samples in [0, maxval] (gray, and Y) and in [-maxval, maxval] (Co, Cg of image.h:53-65).
    rows: (row of the 1-D analysis matrix in y, in x, winning sign) of the coefficient with the largest gray gain;
    crows: the two rows of the one with the largest chroma gain.

    The transform is separable and, rounding aside, linear: the coefficient at (i, j) that the step of depth a
    leaves (encode.c:16-30: rows, then columns, then the same on the LL quadrant) is sum(outer(Ay[i], Ax[j]) * picture)
    with A the analysis matrix of the first a levels.  With p / n the sums of the positive / negative entries of a
    row, the picture that maximises it has maxval where the outer product is positive: P = py*px + ny*nx; the one that
    minimises it gives -N, N = py*nx + ny*px.  Gray gain max(P, N); a signed input reaches P + N."""

    def __init__(self, W, H):
        g = orc.geometry(W, H)
        ws, hs = list(g.widths[:g.levels + 1]), list(g.heights[:g.levels + 1])
        Ax, Ay = np.eye(W), np.eye(H)
        self.gray = self.chroma = 0.0
        self.rows = self.crows = None
        for k in range(g.levels, 0, -1):             # depth g.levels - k + 1 splits the ws[k] x hs[k] LL band
            Ax[:ws[k]] = _step(Ax[:ws[k]])
            Ay[:hs[k]] = _step(Ay[:hs[k]])
            X, Y = Ax[:ws[k]], Ay[:hs[k]]
            px, nx = np.maximum(X, 0).sum(1), np.maximum(-X, 0).sum(1)
            py, ny = np.maximum(Y, 0).sum(1), np.maximum(-Y, 0).sum(1)
            P = np.outer(py, px) + np.outer(ny, nx)
            N = np.outer(py, nx) + np.outer(ny, px)
            P[:hs[k - 1], :ws[k - 1]] = 0              # the LL quadrant is not a coefficient yet (or is the root image)
            N[:hs[k - 1], :ws[k - 1]] = 0
            G = np.maximum(P, N)
            i, j = np.unravel_index(np.argmax(G), G.shape)
            if G[i, j] > self.gray:
                self.gray = float(G[i, j])
                self.rows = (Y[i].copy(), X[j].copy(), 1 if P[i, j] >= N[i, j] else -1)
            S = P + N
            i, j = np.unravel_index(np.argmax(S), S.shape)
            if S[i, j] > self.chroma:
                self.chroma = float(S[i, j])
                self.crows = (Y[i].copy(), X[j].copy())

    def worst_gray(self, M):
        """[H, W, 1]: M where the coefficient's response has the winning sign, 0 elsewhere."""
        ay, ax, sign = self.rows
        return (((sign * np.outer(ay, ax)) > 0) * M).astype(np.uint16)[..., None]

    def worst_rgb(self, M):
        """[H, W, 3]: Co = R - B is +M where the response is positive and -M elsewhere; G = (R + B) / 2."""
        ay, ax = self.crows
        pos = np.outer(ay, ax) > 0
        p = np.empty(pos.shape + (3,), dtype=np.uint16)
        p[..., 0] = np.where(pos, M, 0)
        p[..., 1] = M // 2
        p[..., 2] = np.where(pos, 0, M)
        return p
