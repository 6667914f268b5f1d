"""Delta views, three legs (development aid):
  delta    the delta call: encode_view(cur, base=prev), decode_view(..., base=prev)
  by hand  what a caller writes without it: d = cur.to(int16) - prev.to(int16), encode_view(d, signed=True); a decode into an
           int16 temporary, then (prev.to(int16) + d).clamp(lo, hi).to(dtype)
  plain    the same pictures without a base: encode_view(cur), decode_view(...)
Workloads: 64 gray frames of 4096 x 4096 uint8, 16 gray frames of 4096 x 4096 int16 in [-1024, 3071] and 64 frames of 1920 x
1080 RGB uint8; the base is the synthetic frames of seed i, the picture those of seed i + n (the same scene, other noise).
One process; each leg is warmed up, then the legs take turns `reps` times and every call is timed with HIP events.  Per leg the
peak of torch's allocations above what the legs share is recorded too (the by-hand leg's temporaries).  The decodes' results are
asserted: every leg gives the picture back.  Prints a table and, with an argument, writes it there too ("-": nowhere).
usage: time_delta.py [out.txt [reps]]"""
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


def frames(n, H, W, Cn, lo, hi, seed):
    """[n,H,W,C] in [lo, hi]: the synthetic 8-bit frames of seeds seed .. seed + n - 1 — uint8 as they are, or stretched over
    an int16 range with the bits below filled with noise"""
    pix = ctx.synth_pixels(n, H, W, Cn, seed, 0)
    if (lo, hi) == (0, 255):
        return pix
    k = (hi - lo + 1) // 256
    g = torch.Generator(device=dev).manual_seed(seed)
    x = pix.to(torch.int32) * k + torch.randint(0, k, pix.shape, device=dev, generator=g, dtype=torch.int32) + lo
    return x.to(torch.int16)


def measure(legs):
    """legs: {leg: fn}; -> {leg: (median, min, max, peak MiB)}"""
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
    out = {}
    for k in legs:
        v = sorted(ms[k])
        out[k] = (v[len(v) // 2], v[0], v[-1], peak[k])
    return out


def workload(n, H, W, Cn, lo, hi):
    sgn = lo < 0
    R = hi - lo
    prev, cur = frames(n, H, W, Cn, lo, hi, 0), frames(n, H, W, Cn, lo, hi, n)
    i16 = (lambda t: t) if sgn else (lambda t: t.to(torch.int16))
    out_d, info_d = ctx.encode_view(cur, signed=sgn, base=prev)
    out_p, info_p = ctx.encode_view(cur, signed=sgn)
    out_h, info_h = ctx.encode_view(i16(cur) - i16(prev), signed=True)
    lens_d, lens_p, lens_h = (ctx.stream_lengths(i) for i in (info_d, info_p, info_h))
    assert torch.equal(lens_d, lens_h), "the delta call's streams are not the by-hand residual's"
    bufs = (torch.empty_like(out_d), torch.empty_like(info_d))   # (the encodes' outputs: shared, so that the peaks show the legs' own)
    enc = measure({
        "delta": lambda: ctx.encode_view(cur, out=bufs[0], info=bufs[1], signed=sgn, base=prev),
        "by hand": lambda: ctx.encode_view(i16(cur) - i16(prev), out=bufs[0], info=bufs[1], signed=True),
        "plain": lambda: ctx.encode_view(cur, out=out_p, info=bufs[1], signed=sgn)})   # (8-bit slots are shorter: its own buffer)
    into = torch.empty_like(cur)
    kept = {}
    kw = dict(maxval=hi, signed=sgn, minval=lo if sgn else None)

    def by_hand():
        tmp = torch.empty(cur.shape, dtype=torch.int16, device=dev)
        ctx.decode_view(out_h, lens_h, tmp, maxval=R, minval=-R, signed=True)
        kept["r"] = (i16(prev) + tmp).clamp(lo, hi).to(cur.dtype)

    ctx.decode_view(out_d, lens_d, into, base=prev, **kw)
    assert torch.equal(into, cur), "the delta decode does not give the picture back"
    by_hand()
    assert torch.equal(kept["r"], cur), "the by-hand leg does not give the picture back"
    dec = measure({
        "delta": lambda: ctx.decode_view(out_d, lens_d, into, base=prev, **kw),
        "by hand": by_hand,
        "plain": lambda: ctx.decode_view(out_p, lens_p, into, **kw)})
    assert torch.equal(into, cur), "the plain decode does not give the picture back"
    kept.clear()
    return enc, dec, int(lens_d.sum()), int(lens_p.sum())


lines = ["workload                        call     leg       median ms   min ms   max ms   peak MiB of torch allocations", "-" * 112]
for name, args in (("64 x 4096x4096 gray uint8", (64, 4096, 4096, 1, 0, 255)), ("16 x 4096x4096 gray int16", (16, 4096, 4096, 1, -1024, 3071)),
                   ("64 x 1080p RGB uint8", (64, 1080, 1920, 3, 0, 255))):
    enc, dec, bytes_d, bytes_p = workload(*args)
    torch.cuda.empty_cache()
    for call, rows in (("encode", enc), ("decode", dec)):
        for leg, r in rows.items():
            lines.append("%-31s %-8s %-9s %9.3f %8.3f %8.3f %10.1f" % (name, call, leg, r[0], r[1], r[2], r[3]))
        d, h, p = rows["delta"], rows["by hand"], rows["plain"]
        lines.append("%-31s %-8s delta / by hand: %.3f, delta / plain: %.3f of the time (medians); spread of the repeats: delta %.3f ms, by hand %.3f ms, "
                     "plain %.3f ms" % (name, call, d[0] / h[0], d[0] / p[0], d[2] - d[1], h[2] - h[1], p[2] - p[1]))
    lines.append("%-31s stream bytes: delta %d, plain %d (%.3f)" % (name, bytes_d, bytes_p, bytes_d / bytes_p))
text = "\n".join(lines + ["reps %d, legs alternating, HIP events around each call; decoded samples asserted equal" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
