"""What the encoder's sidecar index costs and what it buys: tools/time_index.py W H C n [calls] [rounds]

Five variants, alternated round by round in one process, each timed with device events around `calls` calls:
  encode            dwtx_encode_device, no index asked for
  encode+index      the same with dwtx_ctx_set_encode_index (device array)
  encode+decode*    the only way to an index without it: the encode and one full decode_device that collects indices
  fresh, no index   encode, then the first decode of the fresh streams the plain way
  fresh, index      encode with the index, its download, then the first decode with the index offered
Prints the median and the spread (min .. max) of the rounds in ms per call."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

W, H, C, n = (int(v) for v in sys.argv[1:5])
calls = int(sys.argv[5]) if len(sys.argv) > 5 else 20
rounds = int(sys.argv[6]) if len(sys.argv) > 6 else 5
ctx = dwt_amd.Context(0)
pix = ctx.synth_pixels(n, H, W, C, 0, 0)
streams, info = ctx.encode_device(pix)
lens = ctx.stream_lengths(info)
back = torch.empty((n, W * H * C), dtype=torch.uint8, device=ctx.device)


def encode():
    ctx.encode_device(pix, out=streams, info=info)


def encode_index():   # (the array is asked for once per timing: what is timed is the encoder)
    ctx.encode_device(pix, out=streams, info=info)


def encode_decode_collecting():
    encode()
    ctx.set_index(None, n)
    ctx.decode_device(streams, lens, W, H, C, out=back)
    ctx.set_index()


def fresh_plain():
    encode()
    ctx.decode_device(streams, lens, W, H, C, out=back)


def fresh_indexed():
    dev = ctx.set_encode_index(n, device=True)
    encode()
    ctx.set_encode_index()
    rows = dev.cpu()   # waits for the encode: the decoder takes its indices from host memory
    offered = (dwt_amd.Index * n).from_buffer_copy(rows.numpy().tobytes())
    ctx.set_index(offered, 0)
    ctx.decode_device(streams, lens, W, H, C, out=back)
    ctx.set_index()


VARIANTS = [("encode", encode), ("encode+index", encode_index), ("encode+decode*", encode_decode_collecting),
            ("fresh, no index", fresh_plain), ("fresh, index", fresh_indexed)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    keep = ctx.set_encode_index(n, device=True) if fn is encode_index else None
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    if keep is not None:
        ctx.set_encode_index()
    return a.elapsed_time(b) / calls


for _, fn in VARIANTS:   # warm up every variant
    timed(fn)
torch.cuda.synchronize()
assert torch.equal(back.view(n, H, W, C), pix), "the indexed decode of the fresh streams is not the picture"
times = {name: [] for name, _ in VARIANTS}
for _ in range(rounds):
    for name, fn in VARIANTS:
        times[name].append(timed(fn))
print(f"{W}x{H}x{C} x{n}: {calls} calls per timing, {rounds} rounds, ms per call: median (min .. max)")
for name, _ in VARIANTS:
    t = times[name]
    print(f"  {name:16s} {statistics.median(t):8.3f}  ({min(t):.3f} .. {max(t):.3f})")
m = {name: statistics.median(t) for name, t in times.items()}
print(f"  index over the plain encode: {1000 * (m['encode+index'] - m['encode']) / n:+.2f} us per frame; "
      f"against encode+decode*: {m['encode+decode*'] - m['encode+index']:.3f} ms saved; "
      f"first decode of fresh streams: {m['fresh, no index'] - m['fresh, index']:+.3f} ms with the index")
