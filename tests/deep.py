"""Deep pixels (samples of more than 8 bits) on the CPU — test infrastructure only.

The reference reads 8-bit PNM and nothing else, but its algorithm does not know the depth: encode.c:155-221 and
decode.c:174-264 work on `int`.  What it would write for wider samples is therefore the composition of the oracle's
depth-agnostic stages, each of which is pinned on the reference by tests/test_oracle.py:

    deep_encode = orc.forward -> orc.linearize -> orc.encode_lin      (after YCoCg-R for colour, image.h:53-65)
    deep_decode = orc.decode_stage -> orc.reconstruct -> orc.inverse  (then image.h:39-51 and pnm.h:108 with the
                                                                       picture's maxval where those have 255)

tests/test_deep_cpu.py checks that the composition equals the whole-file oracle (orc.encode / orc.decode) on 8-bit
pictures and the reference binary's own bytes (tests/golden/smpte*.dwt).

Also here: seeded integer-only generators of deep pictures, and the linear gain model of the transform that says
which depths can never need more than the coder's 16 bit planes."""
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


def deep_decode(data, W, H, C, M, pixels_max=-1, clamp=True):
    """.dwt bytes (or a prefix) -> uint16 [h, w, C] with the clamps at M, or None where decode.c would exit 1.
    clamp=False: int64 samples as the arithmetic leaves them, no clamp anywhere."""
    r = orc.decode_stage(data, W, H, C, pixels_max)
    if r is None:
        return None
    lin, level, missing, planes = r
    img = orc.inverse(orc.reconstruct(lin, W, H, level + 1, missing))
    if not clamp:
        return ycocg2rgb(img, None) if C == 3 else img.astype(np.int64)
    out = ycocg2rgb(img, M) if C == 3 else np.clip(img, 0, M)
    return out.astype(np.uint16)


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
