"""Encode + decode of the RGB of RGBA surfaces (4-byte pixels, of which three are colour), six routes (development aid):
  step         encode_view(rgba[..., :3], stepped=True) / decode_view into the surface: the pixels are coded where they lie
               (8-bit, step 4, everything on the 4-byte grid: lift.hip's Rgbx8 / PIX_STEP4 kernels)
  general      the same calls on the same surface kept one byte off the 4-byte grid: the general conversions
               (k_planes_from_pixels / k_pixels_from_planes) and the int32 transforms
  copies       what the holder had to do before views knew a pixel step: rgba[..., :3].contiguous(), encode_device,
               decode_device and a scattering copy back into the surface
  interleaved  the view of the same pictures kept as dense RGB (what the codec had all along), for scale
  step_bgr     `step` with the same surfaces declared BGRA (order="bgr": the kernels' B, G, R twins); its streams are those of
               the channel-reversed pictures
  copies_bgr   what the holder of a BGRA surface had to do before views knew a channel order: bgra[..., :3].flip(-1) (a
               channel-reversing contiguous copy), encode_device, decode_device and a reversing scatter back
Encode and decode are timed apart, `reps` times, the routes taking turns; every timed call runs under an alarm of its own
(LIMIT seconds: a call that hangs ends the process).  Two workloads: 64 surfaces of 1920 x 1080, and one 4096 x 4096
surface as a 4 x 4 grid of 1024 x 1024 tiles.  Prints one JSON line and, with an argument, writes it there too ("-":
nowhere).  A third argument names the one route to time, for a per-kernel profile.
usage: time_step.py [out.json [reps [route]]]"""
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd
from dwt_amd import tiles

LIMIT = 60
out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
only = sys.argv[3] if len(sys.argv) > 3 else None
ctx = dwt_amd.Context(0)
dev = ctx.device


def timed(fn):
    signal.alarm(LIMIT)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    signal.alarm(0)
    return a.elapsed_time(b)


def surface(shape, off):
    """An RGBA holder of `shape` [..., 4] whose first byte lies `off` bytes into a 4-byte aligned allocation."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.zeros(n + 4, dtype=torch.uint8, device=dev)
    return flat[off:off + n].view(shape)


def workload(name, rgb, windows):
    """rgb: the pictures, dense interleaved [n,H,W,3] or [H,W,3].  windows(t): the view [n,H,W,C] or [rows,cols,H,W,C] of
    the windows of a holder t shaped like rgb, with any channel count."""
    shape4 = tuple(rgb.shape[:-1]) + (4,)
    iview = windows(rgb)
    H, W = iview.shape[-3], iview.shape[-2]
    n = iview.numel() // (H * W * 3)
    src, back = {}, {}
    for route, off in (("step", 0), ("general", 1), ("copies", 0)):
        src[route], back[route] = surface(shape4, off), surface(shape4, off)
        src[route][..., :3] = rgb
        src[route][..., 3] = 0x5A
        back[route][...] = 0xA5
    iback = torch.zeros_like(rgb)
    streams, info = ctx.encode_view(iview)
    stride = (int(ctx.stream_lengths(info).max().item()) * 5 // 4 + 64 + 7) // 8 * 8
    streams = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    dense = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    dback = torch.empty((n, H * W * 3), dtype=torch.uint8, device=dev)

    def lens():
        return ctx.stream_lengths(info)

    def stepped(route, **kw):
        s, b = windows(src[route][..., :3]), windows(back[route][..., :3])
        return (lambda: ctx.encode_view(s, out=streams, info=info, stepped=True, **kw),
                lambda: ctx.decode_view(streams, lens(), b, stepped=True, **kw))

    def copies_enc():
        dense.view(iview.shape).copy_(windows(src["copies"][..., :3]))      # rgba[..., :3].contiguous()
        ctx.encode_device(dense, out=streams, info=info)

    def copies_dec():
        ctx.decode_device(streams, lens(), W, H, 3, out=dback)
        windows(back["copies"][..., :3]).copy_(dback.view(iview.shape))     # and back into the surface

    def copies_bgr_enc():
        ctx.encode_device(windows(src["copies"][..., :3]).flip(-1).contiguous().view(n, H, W, 3), out=streams, info=info)

    def copies_bgr_dec():
        ctx.decode_device(streams, lens(), W, H, 3, out=dback)
        windows(back["copies"][..., :3]).copy_(dback.view(iview.shape).flip(-1))

    routes = {"step": stepped("step"), "general": stepped("general"), "copies": (copies_enc, copies_dec),
              "interleaved": (lambda: ctx.encode_view(iview, out=streams, info=info), lambda: ctx.decode_view(streams, lens(), windows(iback))),
              "step_bgr": stepped("step", order="bgr"), "copies_bgr": (copies_bgr_enc, copies_bgr_dec)}
    surface_of = {"step_bgr": "step", "copies_bgr": "copies"}   # the BGR routes run on their RGB twins' surfaces
    if only:
        routes = {only: routes[only]}
    for enc, dec in routes.values():   # warm-up: scratch, streams, caches
        enc()
        dec()
    res = {k: {"encode": [], "decode": []} for k in routes}
    for _ in range(reps):
        for k, (enc, dec) in routes.items():
            res[k]["encode"].append(round(timed(enc), 3))
            res[k]["decode"].append(round(timed(dec), 3))
    out = {"pictures": n, "W": W, "H": H, "ms_per_call": res}
    if only:
        return out
    keep = {}
    for k, (enc, dec) in routes.items():   # every route: its order's streams, a lossless round trip, the fourth bytes untouched
        b = back.get(surface_of.get(k, k))
        if b is not None:
            b[...] = 0xA5
        enc()
        dec()
        torch.cuda.synchronize()
        order = "bgr" if k in surface_of else "rgb"
        keep.setdefault(order, streams.clone())
        assert torch.equal(streams, keep[order]), name + ": " + k + " gives other streams"
        if k == "interleaved":
            assert torch.equal(iback, rgb), name + ": interleaved round trip"
        else:
            assert torch.equal(b[..., :3], rgb) and bool((b[..., 3] == 0xA5).all()), name + ": " + k + " round trip"
    assert not torch.equal(keep["rgb"], keep["bgr"]), name + ": the order made no difference"
    med = lambda v: sorted(v)[len(v) // 2]
    out["median_ms"] = {k: {"encode": med(r["encode"]), "decode": med(r["decode"]), "both": round(med(r["encode"]) + med(r["decode"]), 3)}
                        for k, r in res.items()}
    out["spread_ms"] = {k: {"encode": round(max(r["encode"]) - min(r["encode"]), 3), "decode": round(max(r["decode"]) - min(r["decode"]), 3)}
                        for k, r in res.items()}
    return out


result = {"reps": reps}

# 64 surfaces of 1080p
frames = ctx.synth_pixels(64, 1080, 1920, 3, 0, 0)
result["rgba_64x1080p"] = workload("rgba_64x1080p", frames, lambda t: t)
del frames
torch.cuda.empty_cache()

# one 4096 x 4096 surface as a 4 x 4 grid of 1024 x 1024 tiles
frame = ctx.synth_pixels(1, 4096, 4096, 3, 7, 0)[0]
g = dwt_amd.tile_groups(4096, 4096, 1024)
assert len(g) == 1
result["rgba_4096_tiles_1024"] = workload("rgba_4096_tiles_1024", frame, lambda t: tiles.group_view(t, g[0]))

line = json.dumps(result)
print(line)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(line + "\n")
