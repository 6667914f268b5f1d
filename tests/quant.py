"""Float sources — test infrastructure only: the picture dwtx_encode_view_float (include/dwtx.h) must code, from the float
samples as they lie in memory, and the float pictures the tests feed it.  Nothing here needs a device.

The reference quantiser, per sample x of colour c: x widened exactly to float32 (float32: as it is; float16 / bfloat16:
torch ON THE CPU, `.float()`), then numpy as two separate operations — `(x * s).astype(np.float32)`, `+ b` — so that nothing
can fuse them, `np.rint` (ties to even), NaN -> 0, `np.clip(0, maxval)`.  scale and bias belong to COLOURS: with order="bgr"
the lowest-addressed sample of a pixel takes scale[2] and bias[2].

The source pictures: given an integer picture p and a (scale, bias), floats of the type near (p + jitter - bias) / scale, with
planted samples at fixed positions of every window (PLANTS).  The expected picture is always quantise(the floats), never p:
the half types cannot hold most of those values, and need not.

Ties.  r = k + 0.5 exactly is reachable in every type with scale 1 (x = k + 0.5) and, for k = 127, with (127.5, 127.5)
(x = 0); with scales that are no powers of two the two roundings land on a tie only by chance — float32 is dense enough for a
search among the neighbours of (k + 0.5 - bias) / scale to find one, the half types are not.  census() counts what a picture
really holds, and tests/test_float_in_cpu.py asserts it per set and type."""
import functools

import numpy as np

import floats

KINDS = floats.KINDS
# the two-roundings witness at scale = bias = 127.5 (tests/test_float_in_cpu.py proves it with exact arithmetic):
# fl32(fl32(x * s) + b) rounds to 20, the single rounding fl32(x * s + b) — a fused multiply-add — to 19
WITNESS = float.fromhex("-0x1.b1b1b2p-1")
UNIT = (127.5, 127.5)


def inverse_of(scale, bias):
    """the (scale, bias) of a decode -> the pair that takes those floats back to the integers: v = f / s - b / s"""
    s, b = floats.three(scale).astype(np.float64), floats.three(bias).astype(np.float64)
    return tuple(1.0 / s), tuple(-b / s)


# name -> maxval -> (scale, bias): the identity, a generator's [-1, 1] (as the README has it), and per colour the inverse
# of floats.SETS["imagenet"] — three different pairs, so that a pair applied to the wrong colour shows
SETS = {"identity": lambda maxval: floats.IDENTITY,
        "unit": lambda maxval: UNIT,
        "imagenet_inv": lambda maxval: inverse_of(*floats.SETS["imagenet"](maxval))}


def widen(bits, kind):
    """bit patterns -> float32, exactly"""
    import torch

    bits = np.array(bits)   # (a contiguous copy of its own: torch wants writable memory, the shared pictures are read-only)
    if kind == "float32":
        return bits.view(np.float32)
    return torch.from_numpy(bits.view(np.int16)).view(floats.torch_dtype(kind)).float().numpy()   # (on the CPU)


def to_bits(x, kind):
    """float64 values -> the bit patterns of the nearest samples of the type"""
    import torch

    with np.errstate(over="ignore"):
        f = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    if kind == "float32":
        return f.view(np.uint32)
    return torch.from_numpy(f).to(floats.torch_dtype(kind)).view(torch.int16).numpy().view(np.uint16)


def rounded(bits, kind, scale, bias, order="rgb"):
    """samples [..., C] as they lie -> r = fl32(fl32(x * s) + b) with the COLOURS R, G, B (or gray) along the last axis"""
    x = widen(bits, kind)
    Cn = x.shape[-1]
    assert Cn in (1, 3) and order in ("rgb", "bgr")
    if order == "bgr" and Cn == 3:
        x = x[..., ::-1]
    s, b = floats.three(scale)[:Cn], floats.three(bias)[:Cn]
    with np.errstate(all="ignore"):
        m = (x * s).astype(np.float32)
        return (m + b).astype(np.float32)


def quantise(bits, kind, scale, bias, maxval, order="rgb"):
    """samples [..., C] as they lie in memory (bit patterns) -> the integers that are coded, colours along the last axis"""
    with np.errstate(all="ignore"):
        q = np.rint(rounded(bits, kind, scale, bias, order))
    q = np.where(np.isnan(q), np.float32(0), q)
    return np.clip(q, 0, maxval).astype(np.int64)


def census(bits, kind, scale, bias, maxval, order="rgb"):
    """what a picture holds of the cases that matter: ties below an even and an odd integer that the clamp leaves alone,
    samples the clamp cuts on either side, NaNs"""
    r = rounded(bits, kind, scale, bias, order).astype(np.float64)
    fin = np.isfinite(r)
    k = np.floor(np.where(fin, r, 0.0))
    tie = fin & (r - k == 0.5) & (k >= 0) & (k + 1 <= maxval)
    return dict(ties_even=int((tie & (k % 2 == 0)).sum()), ties_odd=int((tie & (k % 2 == 1)).sum()),
                low=int((r < -0.5).sum()), high=int((r > maxval + 0.5).sum()), nan=int(np.isnan(r).sum()))


def _neighbours(bits1, kind, reach):
    """the samples around one (same sign, by bit pattern: the next and previous values of the type)"""
    b = int(bits1)
    width = 0xFFFFFFFF if kind == "float32" else 0xFFFF
    c = [b + d for d in range(-reach, reach + 1) if 0 <= (b & (width >> 1)) + d]
    return np.array([v & width for v in c], dtype=floats.BITS[kind])


def tie_sample(kind, s, b, k):
    """a sample x of the type with fl32(fl32(x * s) + b) == k + 0.5 where the search finds one (float32: 64 neighbours on
    either side; the half types: 2), else the sample nearest to (k + 0.5 - b) / s"""
    x0 = to_bits(np.array([(k + 0.5 - float(b)) / float(s)]), kind)
    cand = _neighbours(x0[0], kind, 64 if kind == "float32" else 2)
    r = rounded(cand[:, None], kind, s, b)[:, 0]
    hit = np.flatnonzero(r == np.float32(k + 0.5))
    return cand[hit[0]] if hit.size else x0[0]


# (row, column) of a window -> what lies there, in every channel; columns from the right where negative.  Every window is
# at least 8 x 8.  Rows 2 and 3 reach into the first lane's quad and its neighbour, the last columns into a row's last quad
# and the edge piece before it.
PLANTS = {(2, 1): "tie_even", (2, 2): "tie_odd", (2, 3): "below", (2, 4): "above", (2, 5): "+inf", (2, 6): "-inf", (2, 7): "nan",
          (3, 1): "-0.0", (3, 2): "witness", (3, 4): "tie_even", (4, -1): "nan", (5, -2): "+inf", (5, -1): "below", (6, -4): "-inf",
          (6, 0): "above", (7, 3): "tie_odd"}
SPECIAL = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan, "-0.0": -0.0, "witness": WITNESS}


def source(p, kind, scale, bias, maxval, seed=0, order="rgb"):
    """integer picture p [H, W, C] (colours R, G, B) -> bit patterns [H, W, C] of float samples as they lie in memory
    (order="bgr": B first), near (p + jitter - bias) / scale, with PLANTS in place"""
    H, W, Cn = p.shape
    assert H >= 8 and W >= 8
    s, b = floats.three(scale)[:Cn].astype(np.float64), floats.three(bias)[:Cn].astype(np.float64)
    rng = np.random.default_rng(seed)
    x = (p.astype(np.float64) + rng.uniform(-0.4, 0.4, p.shape) - b) / s
    bits = to_bits(x, kind).copy()
    k_even, k_odd = 2 if maxval >= 3 else 0, 127 if maxval >= 128 else 1   # (2.5 and 127.5: samples of every type; 127.5 is what (127.5, 127.5) reaches with x = 0)
    for (y, col), what in PLANTS.items():
        for c in range(Cn):
            if what in SPECIAL:
                bits[y, col, c] = to_bits(np.array([SPECIAL[what]]), kind)[0]
            elif what == "tie_even":
                bits[y, col, c] = tie_sample(kind, np.float32(s[c]), np.float32(b[c]), k_even)
            elif what == "tie_odd":
                bits[y, col, c] = tie_sample(kind, np.float32(s[c]), np.float32(b[c]), k_odd)
            else:
                r = -7.3 if what == "below" else maxval + 9.6
                bits[y, col, c] = to_bits(np.array([(r - b[c]) / s[c]]), kind)[0]
    return bits[..., ::-1].copy() if order == "bgr" and Cn == 3 else bits


@functools.lru_cache(maxsize=None)
def _base(W, H, Cn, maxval, i):
    """the integer picture the floats of window i are made around (V.picture's: orc.synth, deep.smooth_noise)"""
    import deep
    import orc

    return deep.smooth_noise(W, H, Cn, maxval, seed=i) if maxval > 255 else (orc.synth(W, H, Cn, i, 0).astype(np.int64) * maxval) // 255


@functools.lru_cache(maxsize=None)
def _window(W, H, Cn, kind, maxval, set_name, i, order):
    p = _base(W, H, Cn, maxval, i)
    scale, bias = SETS[set_name](maxval)
    bits = source(p, kind, scale, bias, maxval, seed=i, order=order)
    v = quantise(bits, kind, scale, bias, maxval, order)
    bits.setflags(write=False)
    v.setflags(write=False)
    return bits, v


def window(W, H, Cn, kind, maxval, set_name, i, order="rgb"):
    """window i of a test: (bit patterns [H, W, C] as they lie, the integers [H, W, C] that must be coded); computed once, shared, read-only"""
    return _window(W, H, Cn, kind, maxval, set_name, i, order)


@functools.lru_cache(maxsize=None)
def _oracle(W, H, Cn, kind, maxval, set_name, i, order, capacity):
    import deep
    import orc

    v = _window(W, H, Cn, kind, maxval, set_name, i, order)[1]
    return deep.deep_encode(v.astype(np.uint16), capacity) if maxval > 255 else orc.encode(v.astype(np.uint8), capacity)


def oracle_encode(W, H, Cn, kind, maxval, set_name, i, order="rgb", capacity=0):
    """(.dwt bytes, stats) of window i's integers: orc.encode for maxval <= 255, tests/deep.py's above"""
    return _oracle(W, H, Cn, kind, maxval, set_name, i, order, capacity)
