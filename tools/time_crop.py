"""Crop decode against decode-then-slice (development aid):
  slice     what a caller does without dwtx_decode_view_crop: the plain decode (decode_view, or decode_view_float for the
            float sink) into a full-size NCHW frame, then one `full[i, :, y0:y0+ch, x0:x0+cw]` copy per picture into the
            dense batch of crops — every picture has an origin of its own, so no single strided view describes them
  route 1   decode_view_crop straight into the dense batch, windowed levels (DWTX_OPT_CROP_ROUTE 1)
  route 2   the same call, whole inverse transform and a gather (DWTX_OPT_CROP_ROUTE 2)
  auto      the same call as the library chooses (DWTX_OPT_CROP_ROUTE 0)
Two workloads — 64 gray frames of 4096 x 4096 and 256 RGB frames of 1920 x 1080 — with crops of 1/64, 1/16 and 1/4 of the
area and the whole picture, seeded random origins, into uint8 and float16 NCHW batches.  One process; every leg is warmed
up, then the legs take turns `reps` times and every call is timed with HIP events (all legs end in the decoder's one
synchronisation).  Per leg the peak of torch's allocations above what the legs share (the streams) is recorded too: the
destination, and for `slice` the full-size frame.  Every leg's batch is compared with the slice leg's, bit for bit.
Prints a table and, with an argument, writes it there too ("-": nowhere).
usage: time_crop.py [out.txt [reps [small]]]   (small: a few small frames, to try the tool out)"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
small = len(sys.argv) > 3 and sys.argv[3] == "small"
ctx = dwt_amd.Context(0)
dev = ctx.device
SCALE, BIAS = 1.0 / 255.0, -0.5


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
    del pix, info
    torch.cuda.empty_cache()
    return streams, lens


def workload(name, n, H, W, Cn, seed):
    streams, lens = coded(n, H, W, Cn, seed)
    rows = []
    for dtype in (torch.uint8, torch.float16):
        floats = dtype != torch.uint8
        more = dict(scale=SCALE, bias=BIAS) if floats else {}
        for what, div in (("1/64", 8), ("1/16", 4), ("1/4", 2), ("whole", 1)):
            cw, ch = W // div, H // div
            rng = random.Random(seed * 100 + div)
            origins = [(rng.randint(0, W - cw), rng.randint(0, H - ch)) for _ in range(n)]
            kept = {}

            def slice_leg():
                full = torch.empty((n, Cn, H, W), dtype=dtype, device=dev)
                if floats:
                    ctx.decode_view_float(streams, lens, full.permute(0, 2, 3, 1), **more)
                else:
                    ctx.decode_view(streams, lens, full.permute(0, 2, 3, 1))
                out = torch.empty((n, Cn, ch, cw), dtype=dtype, device=dev)
                for i, (x0, y0) in enumerate(origins):
                    out[i].copy_(full[i, :, y0:y0 + ch, x0:x0 + cw])
                kept["slice"] = out

            def crop_leg(route, key):
                def leg():
                    ctx.set_option("crop_route", route)
                    out = torch.empty((n, Cn, ch, cw), dtype=dtype, device=dev)
                    ctx.decode_view_crop(streams, lens, out.permute(0, 2, 3, 1), (W, H), origins, **more)
                    kept[key] = out
                return leg

            legs = {"slice": slice_leg, "route 1": crop_leg(1, "route 1"), "route 2": crop_leg(2, "route 2"), "auto": crop_leg(0, "auto")}
            peak = {}
            ref = None
            for k, fn in legs.items():   # warm-up (scratch, code objects, torch's allocator), then one call for the peak
                fn()
                kept.clear()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                fn()
                torch.cuda.synchronize()
                peak[k] = (torch.cuda.max_memory_allocated(dev) - before) / 2**20
                bits = torch.int16 if floats else torch.uint8
                if k == "slice":
                    ref = kept[k]
                else:
                    assert torch.equal(kept[k].view(bits), ref.view(bits)), f"{name} {what} {k}: differs from decode-then-slice"
            kept.clear()
            del ref
            ms = {k: [] for k in legs}
            for _ in range(reps):
                for k, fn in legs.items():
                    ms[k].append(timed(fn))
                    kept.clear()
            base = sorted(ms["slice"])
            for k in legs:
                v = sorted(ms[k])
                rows.append("%-18s %-8s %-6s %5dx%-5d %-8s %9.3f %8.3f %8.3f %7.3f %10.1f" % (
                    name, str(dtype).replace("torch.", ""), what, cw, ch, k, v[len(v) // 2], v[0], v[-1], v[len(v) // 2] / base[len(base) // 2], peak[k]))
            torch.cuda.empty_cache()
    ctx.set_option("crop_route", 0)
    return rows


lines = ["workload           sink     crop   size        leg      median ms   min ms   max ms  /slice   peak MiB of torch allocations",
         "-" * 118]
loads = [("64 x 4096^2 gray", 64, 4096, 4096, 1), ("256 x 1080p RGB", 256, 1080, 1920, 3)]
if small:
    loads = [("4 x 520x264 gray", 4, 264, 520, 1), ("4 x 263x135 RGB", 4, 135, 263, 3)]
for name, n, H, W, Cn in loads:
    lines += workload(name, n, H, W, Cn, 11)
text = "\n".join(lines + ["reps %d, legs alternating, HIP events around each call; /slice: median over the slice leg's median" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
