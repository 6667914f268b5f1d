"""Float destinations — test infrastructure only: what dwtx_decode_view_float (include/dwtx.h) must write, from the
integers a CPU decode gives, as BIT PATTERNS (uint32 for float32, uint16 for the two half types): equality of the bits is
the contract, and a frame's fill pattern may well be a NaN.

float32: numpy, as two separate operations — `(v.astype(np.float32) * s).astype(np.float32) + b` — so that nothing can
fuse them.  float16 / bfloat16: that float32 through torch ON THE CPU, `.to(torch.float16 / torch.bfloat16)`: round to
nearest even, overflow to infinity, subnormals kept.  Never the library's own integer decode, and nothing here needs a
device.  tests/test_float_cpu.py holds this helper to hand-computed cases."""
import functools

import numpy as np

KINDS = ("float32", "float16", "bfloat16")
BITS = {"float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16}
IDENTITY = (1.0, 0.0)
# what a classifier's input line does to an 8-bit batch: x / 255, minus the mean, over the deviation — per colour
IMAGENET = (tuple(1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)), tuple(-m / s for m, s in ((0.485, 0.229), (0.456, 0.224), (0.406, 0.225))))
# the same for pictures of another maxval (the deep streams of the tests: 4095)
SETS = {"identity": lambda maxval: IDENTITY,
        "imagenet": lambda maxval: (tuple(s * 255.0 / maxval for s in IMAGENET[0]), IMAGENET[1])}


def three(x):
    """a number or three -> float32[3]"""
    a = np.asarray(x, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    assert a.size == 3
    return a.astype(np.float32)


def torch_dtype(kind):
    import torch

    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[kind]


def reference(v, kind, scale=1.0, bias=0.0, order="rgb"):
    """v: integers [..., C] with the COLOURS R, G, B (or gray) along the last axis, as orc.decode gives them -> the bit
    patterns of the samples as they lie in memory, same shape: with order="bgr" the last axis is reversed AFTER the
    conversion — scale and bias belong to colours, not to memory positions."""
    import torch

    v = np.asarray(v)
    Cn = v.shape[-1]
    assert Cn in (1, 3) and kind in KINDS and order in ("rgb", "bgr")
    s, b = three(scale)[:Cn], three(bias)[:Cn]
    m = (v.astype(np.float32) * s).astype(np.float32)
    f = (m + b).astype(np.float32)
    if kind == "float32":
        bits = f.view(np.uint32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(f)).to(torch_dtype(kind))   # (on the CPU)
        bits = t.view(torch.int16).numpy().view(np.uint16)
    return bits[..., ::-1] if order == "bgr" and Cn == 3 else bits


def fill_bits(samples, kind):
    """A frame's fill, as bit patterns: every value of the type turns up, NaNs and infinities among them, and no two
    neighbours are equal.  (A copy of its own for every caller: the same sizes come again and again.)"""
    return _fill_bits(samples, kind).copy()


@functools.lru_cache(maxsize=8)
def _fill_bits(samples, kind):
    i = np.arange(samples, dtype=np.uint64)
    if kind == "float32":
        return ((i * np.uint64(2654435761) + (i >> np.uint64(7))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return ((i * np.uint64(40503) + (i >> np.uint64(9)) * np.uint64(13) + np.uint64(1)) & np.uint64(0xFFFF)).astype(np.uint16)


def to_device_floats(device, bits, kind):
    """bit patterns (numpy) -> (flat device tensor of the float type, the integer tensor that shares its storage)"""
    import torch

    raw = torch.from_numpy(bits.view(np.int32 if bits.dtype == np.uint32 else np.int16)).to(device)
    return raw.view(torch_dtype(kind)), raw


def bits_of(raw):
    """the integer tensor of to_device_floats -> bit patterns on the host"""
    a = raw.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint16)
