"""Encode + decode of a big gray frame as tiles, through a strided view against a dense copy (development aid).

The frame (default 32768 x 32768, tile 4096: 64 tiles) stays where it is in HBM.  Three ways to code its tiles:
  grid   one dwtx_encode_view / dwtx_decode_view call on the whole 8 x 8 grid
  bands  one call per band of 8 tiles (8 calls each way)
  dense  the tiles copied into a dense batch, dwtx_encode_device / dwtx_decode_device, and the pictures copied back —
         what a caller had to do before there were views; the two copies are timed on their own
Prints one JSON line.  usage: time_views.py [side [tile [reps]]]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd
from dwt_amd import tiles

side = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
tile = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
ctx = dwt_amd.Context(0)
groups = dwt_amd.tile_groups(side, side, tile)
assert len(groups) == 1, "pick a side that is a multiple of the tile: one group, one geometry"
g = groups[0]
n = g.cols * g.rows
frame = ctx.synth_pixels(1, side, side, 1, 0, 0)[0]
back = torch.zeros_like(frame)
view, bview = tiles.group_view(frame, g), tiles.group_view(back, g)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


streams, info = ctx.encode_view(view)
lens = ctx.stream_lengths(info)
stride = (int(lens.max().item()) * 5 // 4 + 64 + 7) // 8 * 8   # rows as wide as the streams need: the decoder's tables follow the stride
streams = torch.empty((n, stride), dtype=torch.uint8, device=frame.device)
ctx.close()
ctx = dwt_amd.Context(0)   # (scratch sized for the worst-case stride goes)
res = {"side": side, "tile": tile, "tiles": n, "reps": reps, "row_pitch": frame.stride(0)}

# grid: one call each way
res["grid_encode_ms"] = timed(lambda: ctx.encode_view(view, out=streams, info=info))
lens = ctx.stream_lengths(info)
res["grid_decode_ms"] = timed(lambda: ctx.decode_view(streams, lens, bview))
assert torch.equal(back, frame), "grid round trip"
grid_streams = streams.clone()

# bands: one call per band
back.zero_()


def enc_bands():
    for r in range(g.rows):
        ctx.encode_view(view[r], out=streams[r * g.cols:(r + 1) * g.cols], info=info[r * g.cols:(r + 1) * g.cols])


def dec_bands():
    for r in range(g.rows):
        ctx.decode_view(streams[r * g.cols:(r + 1) * g.cols], lens[r * g.cols:(r + 1) * g.cols], bview[r])


res["bands_encode_ms"] = timed(enc_bands)
res["bands_decode_ms"] = timed(dec_bands)
assert torch.equal(back, frame), "band round trip"
assert torch.equal(streams, grid_streams), "the band calls write the grid call's streams"

# dense: copy in, the dense entry points, copy out
back.zero_()
dense = torch.empty((n, g.H, g.W, 1), dtype=torch.uint8, device=frame.device)
dview = dense.view(g.rows, g.cols, g.H, g.W, 1)
res["copy_in_ms"] = timed(lambda: dview.copy_(view))
res["dense_encode_ms"] = timed(lambda: ctx.encode_device(dense, out=streams, info=info))
out = dense.view(n, -1)
res["dense_decode_ms"] = timed(lambda: ctx.decode_device(streams, lens, g.W, g.H, 1, out=out))
res["copy_out_ms"] = timed(lambda: bview.copy_(dview))
assert torch.equal(back, frame), "dense round trip"
assert torch.equal(streams, grid_streams), "the dense batch gives the views' streams"

res = {k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}
res["grid_total_ms"] = round(res["grid_encode_ms"] + res["grid_decode_ms"], 3)
res["bands_total_ms"] = round(res["bands_encode_ms"] + res["bands_decode_ms"], 3)
res["dense_total_ms"] = round(res["copy_in_ms"] + res["dense_encode_ms"] + res["dense_decode_ms"] + res["copy_out_ms"], 3)
print(json.dumps(res))
