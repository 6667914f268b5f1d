"""Decode into float tensors, two legs (development aid):
  baseline  what a caller can do without dwtx_decode_view_float: decode_view into a uint8 batch of the same layout, then
            torch's `x.to(dtype) * scale + bias`
  fused     decode_view_float straight into the float batch
Two workloads — 64 frames of 1920 x 1080 RGB, planar ([64,3,1080,1920], the NCHW batch of a training step), and 16 gray
frames of 4096 x 4096 — in float16 and float32.  One process; each leg is warmed up, then the legs take turns `reps` times
and every call is timed with HIP events (both legs end in the decoder's one synchronisation).  Per leg the peak of torch's
allocations above what both legs share (the streams) is recorded too: the pictures, and the temporaries of the torch line.
Prints a table and, with an argument, writes it there too ("-": nowhere).
A third argument, "trace", runs the fused leg alone, each call once, and adds 3 frames of interleaved float RGB — for
rocprofv3 --kernel-trace --stats -- python tools/time_float.py - 1 trace: the planar and the gray calls launch no
k_pixels_from_planes (the inverse transform's last level writes the floats), the interleaved one launches one.
usage: time_float.py [out.txt [reps [trace]]]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
trace = len(sys.argv) > 3 and sys.argv[3] == "trace"
ctx = dwt_amd.Context(0)
dev = ctx.device
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = tuple(1.0 / (255.0 * s) for s in STD)
BIAS = tuple(-m / s for m, s in zip(MEAN, STD))


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def coded(n, H, W, Cn, seed):
    pix = ctx.synth_pixels(n, H, W, Cn, seed, 0)
    streams, info = ctx.encode_device(pix)
    lens = ctx.stream_lengths(info).clone()
    stride = (int(lens.max().item()) + 64 + 7) // 8 * 8
    streams = streams[:, :stride].contiguous()
    ctx.sync()
    return pix, streams, lens


def holder(n, H, W, Cn, dtype, planar):
    """-> (the tensor a caller keeps, its [n,H,W,C] view)"""
    if planar:
        t = torch.empty((n, Cn, H, W), dtype=dtype, device=dev)
        return t, t.permute(0, 2, 3, 1)
    t = torch.empty((n, H, W, Cn), dtype=dtype, device=dev)
    return t, t


def workload(name, n, H, W, Cn, planar, dtype, seed):
    pix, streams, lens = coded(n, H, W, Cn, seed)
    shape = (1, Cn, 1, 1) if planar else (Cn,)
    scale = SCALE[:Cn] if Cn == 3 else SCALE[0]
    bias = BIAS[:Cn] if Cn == 3 else BIAS[0]
    ts = torch.tensor(SCALE[:Cn], dtype=dtype, device=dev).view(shape)
    tb = torch.tensor(BIAS[:Cn], dtype=dtype, device=dev).view(shape)
    kept = {}

    def baseline():
        u8, v8 = holder(n, H, W, Cn, torch.uint8, planar)
        ctx.decode_view(streams, lens, v8)
        kept["baseline"] = u8.to(dtype) * ts + tb

    def fused():
        f, fv = holder(n, H, W, Cn, dtype, planar)
        ctx.decode_view_float(streams, lens, fv, scale=scale, bias=bias)
        kept["fused"] = f

    if trace:
        fused()
        torch.cuda.synchronize()
        return None
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
        kept.clear()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    # what the two legs computed: the fused call is the unfused float32 line, bit for bit, converted once
    u8, v8 = holder(n, H, W, Cn, torch.uint8, planar)
    ctx.decode_view(streams, lens, v8)
    assert torch.equal(v8.reshape(pix.shape), pix), name + ": the integer decode is not lossless"
    ts32 = torch.tensor(SCALE[:Cn], dtype=torch.float32, device=dev).view(shape)   # (the library holds scale and bias as float32, whatever the destination)
    tb32 = torch.tensor(BIAS[:Cn], dtype=torch.float32, device=dev).view(shape)
    want = (u8.float() * ts32 + tb32).to(dtype)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(kept["fused"].view(bits), want.view(bits)), name + ": the fused call differs from the unfused float32 line"
    rows = []
    for k in legs:
        v = sorted(ms[k])
        rows.append((name, str(dtype).replace("torch.", ""), k, v[len(v) // 2], v[0], v[-1], peak[k]))
    kept.clear()
    return rows


lines = ["workload                 dtype    leg       median ms   min ms   max ms   peak MiB of torch allocations",
         "-" * 100]
for dtype in (torch.float16, torch.float32):
    for name, args in (("64 x 1080p RGB planar", (64, 1080, 1920, 3, True)), ("16 x 4096x4096 gray", (16, 4096, 4096, 1, False))):
        rows = workload(name, *args, dtype, 11)
        torch.cuda.empty_cache()
        if rows:
            for r in rows:
                lines.append("%-24s %-8s %-9s %9.3f %8.3f %8.3f %10.1f" % r)
            b, f = rows[0], rows[1]
            lines.append("%-24s %-8s fused / baseline: %.3f of the time (medians), %.3f of the peak; spread of the repeats: baseline %.3f ms, fused %.3f ms"
                         % (name, r[1], f[3] / b[3], f[6] / b[6], b[5] - b[4], f[5] - f[4]))
    if trace:
        workload("3 x 1080p RGB interleaved", 3, 1080, 1920, 3, False, dtype, 11)
text = "\n".join(lines + ["reps %d, legs alternating, HIP events around each call" % reps])
if not trace:
    print(text)
    if out_path and out_path != "-":
        with open(out_path, "w") as f:
            f.write(text + "\n")
