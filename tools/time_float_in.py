"""Encode from float tensors, two legs (development aid):
  baseline  what a caller can do without dwtx_encode_view_float: torch's `(x.float() * s + b).round().clamp(0, maxval)`
            `.to(torch.uint8)` (int16 for maxval 4095), then encode_view of that integer batch in the same layout
  fused     encode_view_float straight from the float batch
The workloads of tools/time_float.py — 64 frames of 1920 x 1080 RGB, planar ([64,3,1080,1920], a generator's NCHW output in
[-1, 1]), and 16 gray frames of 4096 x 4096 — in float16 and float32, quantised to maxval 255 (the 8-bit route) and to 4095
(the deep route): one row per wide source of lift.hip.  One process; each leg is warmed up, then the legs take turns
`reps` times and every call is timed with HIP events.  Per leg the peak of torch's allocations above what both legs share
(the float batch) is recorded too: the outputs, and the temporaries and the integer batch of the torch line.  Both legs
must give identical stream bytes and records, which is asserted.
Prints a table and, with an argument, writes it there too ("-": nowhere).
usage: time_float_in.py [out.txt [reps]]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ctx = dwt_amd.Context(0)
dev = ctx.device


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def floats_of(n, H, W, Cn, planar, dtype, maxval, seed):
    """-> (the float tensor a caller holds, its [n,H,W,C] view): the synthetic frames spread over [-1, 1], with a jitter
    that puts most samples off the integers they came from"""
    pix = ctx.synth_pixels(n, H, W, Cn, seed, 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = pix.float() * (maxval / 255.0) + (torch.rand(pix.shape, device=dev, generator=g) - 0.5) * 0.9
    x = ((x - maxval / 2.0) / (maxval / 2.0)).to(dtype)
    del pix
    if planar:
        t = x.permute(0, 3, 1, 2).contiguous()
        return t, t.permute(0, 2, 3, 1)
    return x, x


def workload(name, n, H, W, Cn, planar, dtype, maxval, seed):
    t, view = floats_of(n, H, W, Cn, planar, dtype, maxval, seed)
    s = b = maxval / 2.0
    itype = torch.uint8 if maxval <= 255 else torch.int16
    kept = {}

    def baseline():
        q = (t.float() * s + b).round().clamp(0, maxval).to(itype)
        kept["baseline"] = ctx.encode_view(q.permute(0, 2, 3, 1) if planar else q)

    def fused():
        kept["fused"] = ctx.encode_view_float(view, maxval=maxval, scale=s, bias=b)

    legs = {"baseline": baseline, "fused": fused}
    peak = {}
    for k, fn in legs.items():   # warm-up (scratch, code objects, torch's allocator), then one call for the peak
        fn()
        kept.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated(dev) - before) / 2**20
        if k == "baseline":
            want = kept["baseline"]
        kept.clear()
    fused()
    torch.cuda.synchronize()
    assert not torch.isnan(t).any()   # (with NaNs torch's clamp and the library's quantiser differ by design)
    # (a slot's bytes behind its stream and the zero padding are left as they were: the streams are compared over their lengths)
    assert torch.equal(kept["fused"][1], want[1]), name + ": the two legs' records differ"
    live = torch.arange(want[0].shape[1], device=dev)[None, :] < ctx.stream_lengths(want[1])[:, None]
    assert torch.equal(kept["fused"][0] * live, want[0] * live), name + ": the two legs' streams differ"
    del live
    del want
    kept.clear()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
            kept.clear()
    rows = []
    for k in legs:
        v = sorted(ms[k])
        rows.append((name, str(dtype).replace("torch.", ""), maxval, k, v[len(v) // 2], v[0], v[-1], peak[k]))
    return rows


lines = ["workload                 dtype    maxval leg       median ms   min ms   max ms   peak MiB of torch allocations",
         "-" * 107]
for maxval in (255, 4095):
    for dtype in (torch.float16, torch.float32):
        for name, args in (("64 x 1080p RGB planar", (64, 1080, 1920, 3, True)), ("16 x 4096x4096 gray", (16, 4096, 4096, 1, False))):
            rows = workload(name, *args, dtype, maxval, 11)
            torch.cuda.empty_cache()
            for r in rows:
                lines.append("%-24s %-8s %6d %-9s %9.3f %8.3f %8.3f %10.1f" % r)
            b, f = rows[0], rows[1]
            lines.append("%-24s %-8s %6d fused / baseline: %.3f of the time (medians), %.3f of the peak; spread of the repeats: baseline %.3f ms, fused %.3f ms"
                         % (name, b[1], maxval, f[4] / b[4], f[7] / b[7], b[6] - b[5], f[6] - f[5]))
text = "\n".join(lines + ["reps %d, legs alternating, HIP events around each call; both legs' streams and records identical" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
