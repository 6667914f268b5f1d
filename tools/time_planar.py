"""Encode + decode of RGB pictures a channel-first holder keeps (NCHW frames, or the tile grid of one CHW frame), three
routes (development aid):
  planar       dwtx_encode_view / dwtx_decode_view on the permuted tensor: the planes are coded where they lie
  copies       what the holder had to do before views knew planes: permute().contiguous(), encode_device, decode_device
               and a permuting copy back into the planes
  interleaved  the view of the same pictures kept channel-last (what the codec had all along)
Each route's encode + decode is timed `reps` times, the routes taking turns.  Two workloads by default: 64 frames of
1920 x 1080, and one 4096 x 4096 frame as a 4 x 4 grid of 1024 x 1024 tiles.  Prints one JSON line and, with an
argument, writes it there too ("-": nowhere).  A fourth argument names the one route to time, for a per-kernel profile:
rocprofv3 --kernel-trace --stats -- python tools/time_planar.py - 3 planar.  usage: time_planar.py [out.json [reps [route]]]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd
from dwt_amd import tiles

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
only = sys.argv[3] if len(sys.argv) > 3 else None
ctx = dwt_amd.Context(0)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def workload(name, nhwc, planar_of, back_of):
    """nhwc: the pictures, interleaved [n,H,W,3] or [rows,cols,H,W,3] (a view of an interleaved holder).  planar_of(t):
    the same pictures in a channel-first holder, as (holder, view).  back_of(): an empty holder of each kind."""
    holder, pview = planar_of(nhwc)
    n = pview.numel() // (pview.shape[-1] * pview.shape[-2] * pview.shape[-3])
    H, W = pview.shape[-3], pview.shape[-2]
    streams, info = ctx.encode_view(pview)
    lens = ctx.stream_lengths(info)
    stride = (int(lens.max().item()) * 5 // 4 + 64 + 7) // 8 * 8
    streams = torch.empty((n, stride), dtype=torch.uint8, device=holder.device)
    pback_holder, pback, iback_holder, iback = back_of()
    dense = torch.empty((n, H, W, 3), dtype=torch.uint8, device=holder.device)
    dback = torch.empty((n, H * W * 3), dtype=torch.uint8, device=holder.device)

    def planar():
        ctx.encode_view(pview, out=streams, info=info)
        ctx.decode_view(streams, ctx.stream_lengths(info), pback)

    def copies():
        dense.view(pview.shape).copy_(pview)                         # permute().contiguous()
        ctx.encode_device(dense, out=streams, info=info)
        ctx.decode_device(streams, ctx.stream_lengths(info), W, H, 3, out=dback)
        pback.copy_(dback.view(pview.shape))                          # and back into the planes

    def interleaved():
        ctx.encode_view(nhwc, out=streams, info=info)
        ctx.decode_view(streams, ctx.stream_lengths(info), iback)

    routes = {"planar": planar, "copies": copies, "interleaved": interleaved}
    if only:
        routes = {only: routes[only]}
    for fn in routes.values():   # warm-up: scratch, streams, caches
        fn()
    res = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            res[k].append(round(timed(fn), 3))
    if only:
        return {"pictures": n, "W": W, "H": H, "ms_per_call": res}
    planar()
    assert torch.equal(pback_holder, holder), name + ": planar round trip"
    keep = streams.clone()
    copies()
    assert torch.equal(pback_holder, holder) and torch.equal(streams, keep), name + ": the copies give the planar view's streams"
    interleaved()
    assert torch.equal(iback, nhwc) and torch.equal(streams, keep), name + ": the interleaved view gives them too"
    return {"pictures": n, "W": W, "H": H, "ms_per_call": res, "median_ms": {k: sorted(v)[len(v) // 2] for k, v in res.items()}}


result = {"reps": reps}

# 64 frames of 1080p: an NCHW batch
frames = ctx.synth_pixels(64, 1080, 1920, 3, 0, 0)


def nchw_of(t):
    holder = t.permute(0, 3, 1, 2).contiguous()
    return holder, holder.permute(0, 2, 3, 1)


def nchw_backs():
    p = torch.zeros((64, 3, 1080, 1920), dtype=torch.uint8, device=frames.device)
    i = torch.zeros_like(frames)
    return p, p.permute(0, 2, 3, 1), i, i


result["nchw_64x1080p"] = workload("nchw", frames, nchw_of, nchw_backs)
del frames
torch.cuda.empty_cache()

# one 4096 x 4096 frame, CHW, as a 4 x 4 grid of 1024 x 1024 tiles
frame = ctx.synth_pixels(1, 4096, 4096, 3, 7, 0)[0]
g = dwt_amd.tile_groups(4096, 4096, 1024)
assert len(g) == 1
g = g[0]


def chw_of(t):
    holder = frame.permute(2, 0, 1).contiguous()
    return holder, tiles.group_view(holder.permute(1, 2, 0), g)


def chw_backs():
    p = torch.zeros((3, 4096, 4096), dtype=torch.uint8, device=frame.device)
    i = torch.zeros_like(frame)
    return p, tiles.group_view(p.permute(1, 2, 0), g), i, tiles.group_view(i, g)


def chw_workload():
    view = tiles.group_view(frame, g)
    r = workload("chw_tiles", view, chw_of, chw_backs)
    return r


result["chw_4096_tiles_1024"] = chw_workload()
line = json.dumps(result)
print(line)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(line + "\n")
