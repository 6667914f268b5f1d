"""Every view entry point once, for a kernel trace (development aid).  On one context, for each of the
shapes gray 72 x 68, gray 256 x 256 and RGB 520 x 264 — one below and two above the wide kernels' threshold, the shapes of
profiles/flip_kernel_calls.txt — and four pictures a call, one encode and one decode
  through each view entry point with an argument that is not its neutral value: view, step, order, float, crop, list, flip,
    signed, delta, chain;
  through each call that is, by include/dwtx.h, another call with fewer arguments: the flip calls with all flags 0 on a grid
    and on a list, the crop call with the whole picture, the signed calls with a float format and minval 0, the chain calls
    with n = 1, the step calls with pixel_step == channels.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/view_calls.py` (kernel trace only) on two builds: the launch
counts per kernel say which route every call took, and two builds that route alike give the same counts line for line.
Every integer result is compared with its source, so a run that ends is also a round trip of every entry.
usage: view_calls.py"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd
from dwt_amd import DecodeInfo, StreamInfo, View, float_format

N = 4
ctx = dwt_amd.Context(0)
dev, lib, h = ctx.device, ctx.lib, ctx.h
legs = []


def ptr(t):
    return C.c_void_p(t.data_ptr())


def lens_of(info):
    return ctx.stream_lengths(info).clone()


def leg(name, got, want):
    ctx.sync()
    assert torch.equal(got, want), f"{name}: the decode differs from the source"
    legs.append(name)


def raw_view(t, maxval):
    """a dense [n,H,W,C] tensor as a dwtx_view"""
    n, H, W, Cn = t.shape
    return View(t.data_ptr(), t.element_size(), Cn, maxval, 0, W * Cn, H * W * Cn, 0, 0)


def raw_encode(sym, t, before, after=(), bound16=False):
    """lib.<sym>(ctx, view, *before, W, H, n, capacity, out, stride, info) -> (streams, lens)"""
    n, H, W, Cn = t.shape
    stride = (lib.dwtx_encode_bound16 if bound16 else lib.dwtx_encode_bound)(W, H, Cn)
    out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    info = torch.empty((n, C.sizeof(StreamInfo)), dtype=torch.uint8, device=dev)
    rc = getattr(lib, sym)(h, *before, *after, W, H, n, 0, ptr(out), stride, ptr(info))
    assert rc == 0, (sym, rc, lib.dwtx_last_error())
    return out, lens_of(info)


def raw_decode(sym, streams, lens, into, args):
    """lib.<sym>(ctx, streams, stride, lens, W, H, n, levels_max, *args, infos)"""
    n, H, W, Cn = into.shape
    infos = (DecodeInfo * n)()
    rc = getattr(lib, sym)(h, ptr(streams), streams.shape[1], ptr(lens), W, H, n, -1, *args, C.cast(infos, C.c_void_p))
    assert rc == 0, (sym, rc, lib.dwtx_last_error())
    return into


def shape_calls(W, H, Cn):
    tag = f"{'gray' if Cn == 1 else 'rgb'} {W}x{H}"
    pix = ctx.synth_pixels(N, H, W, Cn, 7, 0)
    new = lambda like=pix: torch.zeros_like(like)   # noqa: E731

    # -- each entry with an argument of its own --------------------------------------------------------------------------
    s, i = ctx.encode_view(pix)
    leg(f"{tag} view", ctx_decode(s, i, new()), pix)

    wide = torch.zeros((N, H, W, Cn + 1), dtype=torch.uint8, device=dev)   # RGBA, or gray + alpha
    wide[..., :Cn] = pix
    s, i = ctx.encode_view(wide[..., :Cn], stepped=True)
    back = torch.zeros_like(wide)
    ctx.decode_view(s, lens_of(i), back[..., :Cn], stepped=True)
    leg(f"{tag} step", back, wide)

    s, i = ctx.encode_view(pix, order="bgr")
    back = new()
    ctx.decode_view(s, lens_of(i), back, order="bgr")
    leg(f"{tag} order", back, pix)

    x = pix.to(torch.float32)
    s, i = ctx.encode_view_float(x)
    back = torch.zeros_like(x)
    ctx.decode_view_float(s, lens_of(i), back)
    leg(f"{tag} float", back, x)

    s, i = ctx.encode_view(pix)
    cw, ch = W // 2, H // 2
    back = torch.zeros((N, ch, cw, Cn), dtype=torch.uint8, device=dev)
    ctx.decode_view_crop(s, lens_of(i), back, (W, H), (3, 5))
    leg(f"{tag} crop", back, pix[:, 5:5 + ch, 3:3 + cw])

    wins = [pix[k] for k in (2, 0, 3, 1)]
    s, i = ctx.encode_view_list(wins)
    back = new()
    ctx.decode_view_list(s, lens_of(i), [back[k] for k in (2, 0, 3, 1)])
    leg(f"{tag} list", back, pix)

    for key in ("y", "x"):
        s, i = ctx.encode_view(pix, flip=key)
        back = new()
        ctx.decode_view(s, lens_of(i), back, flip=key)
        leg(f"{tag} flip {key}", back, pix)

    sig = pix.to(torch.int16) * 16 - 2000
    s, i = ctx.encode_view(sig, signed=True)
    back = torch.zeros_like(sig)
    ctx.decode_view(s, lens_of(i), back, signed=True)
    leg(f"{tag} signed", back, sig)

    base = ctx.synth_pixels(N, H, W, Cn, 9, 0)
    s, i = ctx.encode_view(pix, base=base)
    back = new()
    ctx.decode_view(s, lens_of(i), back, base=base)
    leg(f"{tag} delta", back, pix)

    s, i = ctx.encode_view_chain(pix, base[0])
    back = new()
    ctx.decode_view_chain(s, lens_of(i), back, base[0])
    leg(f"{tag} chain", back, pix)

    # -- each call that is another call with fewer arguments -------------------------------------------------------------
    v = raw_view(pix, 255)
    arr = (C.c_void_p * N)(*[pix[k].data_ptr() for k in range(N)])
    zeros = (C.c_ubyte * N)(0, 0, 0, 0)
    for what, windows, flips in (("grid", None, None), ("list", arr, zeros)):
        s, ln = raw_encode("dwtx_encode_view_flip", pix, (C.byref(v), 0, 0, None, windows, 0, flips))
        back = new()
        vb = raw_view(back, 255)
        barr = None if windows is None else (C.c_void_p * N)(*[back[k].data_ptr() for k in range(N)])
        raw_decode("dwtx_decode_view_flip", s, ln, back, (C.byref(vb), 0, 0, None, W, H, None, barr, 0, flips))
        leg(f"{tag} flip call, all flags 0, {what}", back, pix)

    s, i = ctx.encode_view(pix)
    back = new()
    ctx.decode_view_crop(s, lens_of(i), back, (W, H))
    leg(f"{tag} crop call, whole picture", back, pix)

    x = pix.to(torch.float32)
    fmt = float_format(torch.float32, 1.0, 0.0)
    vx = raw_view(x, 255)
    s, ln = raw_encode("dwtx_encode_view_signed", x, (C.byref(vx), 0, 0, C.byref(fmt), None, 0, None, 0))
    back = torch.zeros_like(x)
    vb = raw_view(back, 255)
    raw_decode("dwtx_decode_view_signed", s, ln, back, (C.byref(vb), 0, 0, C.byref(fmt), W, H, None, None, 0, None, 0))
    leg(f"{tag} signed call, float format and minval 0", back, x)

    s, i = ctx.encode_view_chain(pix[:1], base[0])
    back = new(pix[:1])
    ctx.decode_view_chain(s, lens_of(i), back, base[0])
    leg(f"{tag} chain calls, n = 1", back, pix[:1])

    s, ln = raw_encode("dwtx_encode_view_step", pix, (C.byref(v), Cn))
    back = new()
    vb = raw_view(back, 255)
    raw_decode("dwtx_decode_view_step", s, ln, back, (C.byref(vb), Cn))
    leg(f"{tag} step call, pixel_step == channels", back, pix)


def ctx_decode(streams, info, into):
    ctx.decode_view(streams, lens_of(info), into)
    return into


for W, H, Cn in ((72, 68, 1), (256, 256, 1), (520, 264, 3)):
    shape_calls(W, H, Cn)
ctx.sync()
ctx.close()
print("\n".join(legs))
print(f"{len(legs)} legs, each one encode and one decode of {N} pictures")
