"""decode_view_clips_crop against what a caller writes without it (development aid).  Per workload and case
two legs:
  fused   decode_view_clips_crop(streams, lens, into, period, size, origins, scale=, bias=): crop-sized windows, float or integer
  parent  decode_view_clips into a full-size integer stack, then the slice per clip, then — for a float destination —
          `.float() * scale + bias` and `.to(dtype)`
Cases: crops of 1/4 and 1/16 of the area into float16 (the loader's two lines together), the integer crop alone (1/4), and the
float sink alone (full size, float16).  One origin per clip, seeded.
Workloads: section 4.24's — 64 clips of 16 frames of 224 x 224 RGB uint8 (n = 1024, period 16), 8 volumes of 64 slices of 512 x
512 int16 in [-1024, 3071] (n = 512, period 64) and 64 frames of 1920 x 1080 RGB uint8 with period 8.
One process; each leg is warmed up, then the legs take turns `reps` times, timed with the host's clock from a synchronised device
to a final synchronise.  The two legs' results are asserted equal, bit for bit.  Memory: the destination both legs end with, and
the temporaries of each leg — torch's peak allocation above what is live before the leg (the library's own scratch, which both
legs share through the int32 pyramid, is not torch's and is not counted; the fused leg adds two carry pictures of the crop's
size to it).  Prints a table and, with an argument, writes it there too ("-": nowhere).
usage: time_clips_crop.py [out.txt [reps [workload index]]]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
only = int(sys.argv[3]) if len(sys.argv) > 3 else -1
ctx = dwt_amd.Context(0)
dev = ctx.device
SCALE, BIAS = (1 / 58.4, 1 / 57.1, 1 / 57.4), (-2.12, -2.04, -1.80)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def frames(n, H, W, Cn, lo, hi):
    """tools/time_clips.py's frames"""
    pix = ctx.synth_pixels(n, H, W, Cn, 0, 0)
    if (lo, hi) == (0, 255):
        return pix
    k = (hi - lo + 1) // 256
    g = torch.Generator(device=dev).manual_seed(1)
    x = pix.to(torch.int32) * k + torch.randint(0, k, pix.shape, device=dev, generator=g, dtype=torch.int32) + lo
    return x.to(torch.int16)


def measure(legs):
    """legs: {leg: fn}; -> {leg: (median, min, max)} in ms"""
    for fn in legs.values():   # warm-up: scratch, code objects, torch's allocator
        fn()
        fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    out = {}
    for k in legs:
        v = sorted(ms[k])
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


def peak_above(fn):
    """torch's peak allocation during fn above what was live before it, in bytes"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def workload(n, H, W, Cn, lo, hi, period):
    sgn = lo < 0
    t = frames(n, H, W, Cn, lo, hi)
    out, info = ctx.encode_view_clips(t, period, signed=sgn)
    lens = ctx.stream_lengths(info)
    del info
    kw = dict(maxval=hi, signed=sgn, minval=lo if sgn else None)
    nclips = -(-n // period)
    scale, bias = (SCALE, BIAS) if Cn == 3 else (SCALE[0], BIAS[0])
    sc = torch.tensor(SCALE[:Cn], dtype=torch.float32, device=dev)
    bi = torch.tensor(BIAS[:Cn], dtype=torch.float32, device=dev)
    rows = []
    for case, (cw, ch), dtype in (("crop 1/4 -> float16", (W // 2, H // 2), torch.float16), ("crop 1/16 -> float16", (W // 4, H // 4), torch.float16),
                                  ("crop 1/4, integer", (W // 2, H // 2), None), ("full size -> float16", (W, H), torch.float16)):
        g = torch.Generator().manual_seed(7)
        org = [(int(torch.randint(0, W - cw + 1, (1,), generator=g)), int(torch.randint(0, H - ch + 1, (1,), generator=g))) for _ in range(nclips)]
        into = torch.zeros((n, ch, cw, Cn), dtype=dtype or t.dtype, device=dev)
        theirs = torch.zeros_like(into)
        fkw = dict(scale=scale, bias=bias, maxval=hi, minval=lo) if dtype else kw

        def fused():
            ctx.decode_view_clips_crop(out, lens, into, period, (W, H), org, **fkw)

        def parent():
            full = torch.empty_like(t)
            ctx.decode_view_clips(out, lens, full, period, **kw)
            for k, (x0, y0) in enumerate(org):
                cut = full[k * period:(k + 1) * period, y0:y0 + ch, x0:x0 + cw]
                theirs[k * period:(k + 1) * period] = (cut.float() * sc + bi).to(dtype) if dtype else cut

        fused()
        parent()
        raw = torch.int16 if into.element_size() == 2 else torch.uint8
        assert torch.equal(into.view(raw), theirs.view(raw)), f"{case}: the two legs differ"
        mem = {"fused": peak_above(fused), "parent": peak_above(parent)}
        r = measure({"fused": fused, "parent": parent})
        rows.append((case, r, into.numel() * into.element_size(), mem))
        del into, theirs
        torch.cuda.empty_cache()
    return rows


def spread(r):
    return r[2] - r[1]


WORKLOADS = (("64 clips x 16 x 224x224 RGB uint8", (1024, 224, 224, 3, 0, 255, 16)), ("8 volumes x 64 x 512x512 int16", (512, 512, 512, 1, -1024, 3071, 64)),
             ("64 x 1080p RGB uint8, period 8", (64, 1080, 1920, 3, 0, 255, 8)))
MiB = 1024.0 * 1024.0
lines = ["workload                            case                   leg      median ms   min ms   max ms   dest MiB   temp MiB", "-" * 112]
for k, (name, args) in enumerate(WORKLOADS):
    if only >= 0 and k != only:
        continue
    for case, r, dest, mem in workload(*args):
        for leg in ("fused", "parent"):
            v = r[leg]
            lines.append("%-35s %-22s %-8s %9.3f %8.3f %8.3f %10.2f %10.2f" % (name, case, leg, v[0], v[1], v[2], dest / MiB, mem[leg] / MiB))
        f, p = r["fused"], r["parent"]
        verdict = "faster" if p[0] - f[0] > spread(f) + spread(p) else "NOT FASTER (the medians lie within the spread)" if abs(p[0] - f[0]) <= spread(f) + spread(p) else "SLOWER"
        lines.append("%-35s %-22s fused / parent: %.3f of the time (medians); parent - fused: %.3f ms; spread of the repeats: fused %.3f ms, parent %.3f ms: %s" %
                     (name, case, f[0] / p[0], p[0] - f[0], spread(f), spread(p), verdict))
    torch.cuda.empty_cache()
text = "\n".join(lines + ["reps %d, legs alternating, host clock from a synchronised device to a final synchronise; both legs' results asserted equal bit for bit; "
                          "temp: torch's peak allocation during a leg above what is live before it" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
