"""Signed 16-bit pictures, three legs (development aid):
  signed    the signed call: encode_view(x, signed=True), decode_view(..., signed=True, minval=, maxval=), decode_view_float(..., minval=)
  shift     what a caller does without it: encode_view(x - minval); decode_view into a temporary, then `+ minval` (and
            `.half() * s + b` for a float16 destination)
  unsigned  the unsigned call on the picture that is already shifted, the shift itself not counted
Workloads: 16 gray frames of 4096 x 4096 in [-1024, 3071] and 64 frames of 1920 x 1080 RGB in [-2048, 2047], each as an encode,
as a decode into int16 and as a decode into float16.  One process; each leg is warmed up, then the legs take turns `reps`
times and every call is timed with HIP events.  Per leg the peak of torch's allocations above what the legs share is recorded
too.  The decodes' results are asserted: the signed and the shift leg give the picture back, the unsigned leg the shifted one.
Prints a table and, with an argument, writes it there too ("-": nowhere).
usage: time_signed.py [out.txt [reps]]"""
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


def picture(n, H, W, Cn, lo, hi, seed):
    """int16 [n,H,W,C] in [lo, hi]: the synthetic 8-bit frames stretched over the range, the bits below filled with noise"""
    k = (hi - lo + 1) // 256
    pix = ctx.synth_pixels(n, H, W, Cn, seed, 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = pix.to(torch.int32) * k + torch.randint(0, k, pix.shape, device=dev, generator=g, dtype=torch.int32) + lo
    return x.to(torch.int16)


def measure(name, what, legs):
    """legs: {leg: fn}; -> rows (name, what, leg, median, min, max, peak MiB)"""
    peak = {}
    for k, fn in legs.items():   # warm-up (scratch, code objects, torch's allocator), then one call for the peak
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated(dev) - before) / 2**20
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    rows = []
    for k in legs:
        v = sorted(ms[k])
        rows.append((name, what, k, v[len(v) // 2], v[0], v[-1], peak[k]))
    return rows


def workload(name, n, H, W, Cn, lo, hi, seed):
    R = hi - lo
    x = picture(n, H, W, Cn, lo, hi, seed)
    xs = x - lo                     # the shifted picture: values in [0, R], carried in int16 as the unsigned calls take them
    assert int(x.min()) < 0 < int(x.max()) and int(xs.min()) >= 0 and int(xs.max()) <= R
    s, b = 1.0 / 1024, 0.5
    out_s, info_s = ctx.encode_view(x, signed=True)
    out_u, info_u = ctx.encode_view(xs)
    lens_s, lens_u = ctx.stream_lengths(info_s), ctx.stream_lengths(info_u)
    into, f16 = torch.empty_like(x), torch.empty(x.shape, dtype=torch.float16, device=dev)
    bufs = (torch.empty_like(out_s), torch.empty_like(info_s))   # (the encodes' outputs: shared, so that the peaks show the legs' own)
    rows = []
    rows += measure(name, "encode", {
        "signed": lambda: ctx.encode_view(x, out=bufs[0], info=bufs[1], signed=True),
        "shift": lambda: ctx.encode_view(x - lo, out=bufs[0], info=bufs[1]),
        "unsigned": lambda: ctx.encode_view(xs, out=bufs[0], info=bufs[1])})
    kept = {}

    def shift_i16():
        tmp = torch.empty_like(x)
        ctx.decode_view(out_u, lens_u, tmp, maxval=R)
        kept["r"] = tmp + lo

    def shift_f16():
        tmp = torch.empty_like(x)
        ctx.decode_view(out_u, lens_u, tmp, maxval=R)
        kept["r"] = (tmp + lo).half() * s + b

    ctx.decode_view(out_s, lens_s, into, maxval=hi, minval=lo, signed=True)
    assert torch.equal(into, x), name + ": the signed decode does not give the picture back"
    shift_i16()
    assert torch.equal(kept["r"], x), name + ": the shift leg does not give the picture back"
    rows += measure(name, "decode int16", {
        "signed": lambda: ctx.decode_view(out_s, lens_s, into, maxval=hi, minval=lo, signed=True),
        "shift": shift_i16,
        "unsigned": lambda: ctx.decode_view(out_u, lens_u, into, maxval=R)})
    assert torch.equal(into, xs), name + ": the unsigned decode does not give the shifted picture back"
    kept.clear()
    ctx.decode_view_float(out_s, lens_s, f16, maxval=hi, minval=lo, scale=s, bias=b)
    shift_f16()
    assert torch.equal(f16, kept["r"]), name + ": the signed float16 decode and the shift leg differ"
    kept.clear()
    rows += measure(name, "decode float16", {
        "signed": lambda: ctx.decode_view_float(out_s, lens_s, f16, maxval=hi, minval=lo, scale=s, bias=b),
        "shift": shift_f16,
        "unsigned": lambda: ctx.decode_view_float(out_u, lens_u, f16, maxval=R, scale=s, bias=b)})
    kept.clear()
    return rows


lines = ["workload                 range          call           leg       median ms   min ms   max ms   peak MiB of torch allocations",
         "-" * 121]
for name, args in (("16 x 4096x4096 gray", (16, 4096, 4096, 1, -1024, 3071)), ("64 x 1080p RGB", (64, 1080, 1920, 3, -2048, 2047))):
    rows = workload(name, *args, 11)
    torch.cuda.empty_cache()
    rng = "%d..%d" % args[4:6]
    for i in range(0, len(rows), 3):
        g, sh, u = rows[i:i + 3]
        for r in (g, sh, u):
            lines.append("%-24s %-14s %-14s %-9s %9.3f %8.3f %8.3f %10.1f" % (r[0], rng, r[1], r[2], r[3], r[4], r[5], r[6]))
        lines.append("%-24s %-14s %-14s signed / unsigned: %.3f, signed / shift: %.3f of the time (medians); spread of the repeats: signed %.3f ms, "
                     "shift %.3f ms, unsigned %.3f ms" % (g[0], rng, g[1], g[3] / u[3], g[3] / sh[3], g[5] - g[4], sh[5] - sh[4], u[5] - u[4]))
text = "\n".join(lines + ["reps %d, legs alternating, HIP events around each call; decoded samples asserted equal" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
