"""Two builds of libdwtx.so, the pixel conversions of both, byte for byte (development aid).
Both libraries are loaded into this one process (each with its own symbols: RTLD_LOCAL), each gets a context, and every
case runs in both on equal inputs into destinations that were filled with the same seeded bytes; the destinations are
compared whole: the samples the calls write and everything around them that they must not.
  the four exported conversions, 70 x 67, gray and RGB, 5 windows:
    dwtx_pixels_from_planes / dwtx_pixels16_from_planes (maxval 255 / 1023 and 65535) on seeded int32 planes drawn from
    +-3 * 65535, so that every input and output clamp acts; dwtx_planes_from_pixels / dwtx_planes_from_pixels16 on seeded
    pixels of the whole range
  the delta, chain and clips view decodes, uint8 / uint16 / int16, gray and RGB, on streams that library A made from such
    pictures, whole and cut to 0.7 of their lengths (lossy residuals: the clamps act): delta of 5 windows, chains of 1, 3,
    4, 5 and 9, clips of 11 windows with periods 2 and 3, decoded as one group (one_stream: it starts at its key) and in 2
    and 4 parts (groups from windows 5, and 2, 5 and 8: mid-clip for one period or both); each into a window of a larger,
    seeded tensor.
Prints one line per case and exits 1 if any differs.
usage: conv_diff.py A/libdwtx.so B/libdwtx.so"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dwt_amd
from dwt_amd import _lib

W, H, N = 70, 67, 5
DEV = torch.device("cuda", 0)


def context_of(path):
    """a dwt_amd.Context on the library at `path` instead of the package's own"""
    lib = C.CDLL(os.path.abspath(path))   # (RTLD_LOCAL: the second library's calls bind to its own functions)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    ctx = dwt_amd.Context.__new__(dwt_amd.Context)
    ctx.torch, ctx.lib, ctx.device = torch, lib, DEV
    h = C.c_void_p()
    rc = lib.dwtx_ctx_create_on_stream(0, torch.cuda.current_stream(DEV).cuda_stream, C.byref(h))
    assert rc == 0, f"dwtx_ctx_create_on_stream of {path}: {rc}"
    ctx.h = h
    return ctx


def seeded(shape, dtype, seed, lo=None, hi=None):
    """a device tensor of seeded samples: the whole range of dtype, or [lo, hi]"""
    info = np.iinfo(dtype)
    a = np.random.default_rng(seed).integers(info.min if lo is None else lo, (info.max if hi is None else hi) + 1, size=shape, dtype=np.int64)
    return torch.from_numpy(a.astype(dtype)).to(DEV)


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


results = []


def case(name, run):
    """run(ctx) -> the tensors the case wrote into; once per library"""
    outs = [run(ctx) for ctx in ctxs]
    torch.cuda.synchronize()
    ok = all(same(x, y) for x, y in zip(*outs))
    results.append(ok)
    print("%-72s %s  (%d bytes compared)" % (name, "equal" if ok else "DIFFERENT", sum(x.numel() * x.element_size() for x in outs[0])))


def conversions():
    for Cn in (1, 3):
        planes = seeded((N * Cn, H, W), np.int32, 10 + Cn, -3 * 65535, 3 * 65535)
        for maxval in (255, 1023, 65535):
            for deep in ((False, True) if maxval == 255 else (True,)):
                def run(ctx, deep=deep, maxval=maxval):
                    out = seeded((N * H * W * Cn + 64,), np.uint16 if deep else np.uint8, 20)   # (64 samples past the end: not written)
                    args = (ctx.h, out.data_ptr(), planes.data_ptr(), W, H, Cn, N)
                    rc = ctx.lib.dwtx_pixels16_from_planes(*args, maxval) if deep else ctx.lib.dwtx_pixels_from_planes(*args)
                    assert rc == 0, rc
                    ctx.sync()
                    return [out]
                case("pixels%s_from_planes  C=%d maxval %d" % ("16" if deep else "", Cn, maxval), run)
        for deep in (False, True):
            pix = seeded((N, H, W, Cn), np.uint16 if deep else np.uint8, 30 + Cn)

            def run(ctx, deep=deep, pix=pix):
                out = seeded((N * Cn * H * W + 64,), np.int32, 40)
                fn = ctx.lib.dwtx_planes_from_pixels16 if deep else ctx.lib.dwtx_planes_from_pixels
                rc = fn(ctx.h, out.data_ptr(), pix.data_ptr(), W, H, Cn, N)
                assert rc == 0, rc
                ctx.sync()
                return [out]
            case("planes_from_pixels%s  C=%d" % ("16" if deep else "", Cn), run)


KINDS = (("u8", np.uint8, False, None, None), ("u16", np.uint16, False, None, None), ("s16", np.int16, True, -32768, 32767))


def window(n, Cn, dtype, seed):
    """n windows of W x H inside a larger seeded tensor, which is what gets compared"""
    big = seeded((n, H + 3, W + 5, Cn), dtype, seed)
    return big, big[:, :H, :W, :]


def views():
    A = ctxs[0]
    for kind, dtype, sgn, lo, hi in KINDS:
        kw = dict(signed=sgn, minval=lo, maxval=hi) if sgn else {}
        for Cn in (1, 3):
            pics = seeded((12, H, W, Cn), dtype, 50 + Cn)   # picture 0: the base, or the key
            for cut in (1.0, 0.7):
                def lens_of(info):
                    lens = A.stream_lengths(info)
                    return lens if cut == 1.0 else (lens.to(torch.float64) * cut).to(torch.int64)
                tag = "%s C=%d %s" % (kind, Cn, "whole" if cut == 1.0 else "cut 0.7")
                out, info = A.encode_view(pics[1:1 + N], base=pics[:N], signed=sgn)
                lens = lens_of(info)

                def run(ctx, out=out, lens=lens):
                    big, into = window(N, Cn, dtype, 60)
                    ctx.decode_view(out, lens, into, base=pics[:N], **kw)
                    return [big]
                case("decode_view_delta  %s, %d windows" % (tag, N), run)
                for n in (1, 3, 4, 5, 9):
                    out, info = A.encode_view_chain(pics[1:1 + n], pics[0], signed=sgn)
                    lens = lens_of(info)

                    def run(ctx, out=out, lens=lens, n=n):
                        big, into = window(n, Cn, dtype, 61)
                        ctx.decode_view_chain(out, lens, into, pics[0], **kw)
                        return [big]
                    case("decode_view_chain  %s, %d windows" % (tag, n), run)
                for period in (2, 3):
                    out, info = A.encode_view_clips(pics[:11], period, signed=sgn)
                    lens = lens_of(info)
                    for parts in (1, 2, 4):   # the groups begin at windows 0; 0, 5; 0, 2, 5, 8
                        def run(ctx, out=out, lens=lens, period=period, parts=parts):
                            big, into = window(11, Cn, dtype, 62)
                            ctx.set_option("one_stream", parts == 1)
                            ctx.set_option("decode_parts", parts)
                            ctx.decode_view_clips(out, lens, into, period, **kw)
                            ctx.set_option("one_stream", 0)
                            ctx.set_option("decode_parts", 0)
                            return [big]
                        case("decode_view_clips  %s, 11 windows, period %d, %s" % (tag, period, "one group, from its key" if parts == 1 else "%d groups, some from mid-clip" % parts), run)


if len(sys.argv) != 3:
    sys.exit(__doc__)
ctxs = [context_of(p) for p in sys.argv[1:3]]
print("A %s\nB %s" % tuple(os.path.abspath(p) for p in sys.argv[1:3]))
conversions()
views()
print("%d cases, %d equal, %d different" % (len(results), sum(results), len(results) - sum(results)))
sys.exit(0 if all(results) else 1)
