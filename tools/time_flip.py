"""Flips in views against flip-by-copy (development aid).  Three pairs, the copy leg first:
  encode       copy   torch.flip(x, [rows]) of the bottom-up batch, then encode_view
               flip   encode_view(flip="y") of the batch as it lies
  decode       copy   decode_view_float into a planar float16 batch [N,3,H,W] with scale and bias, then the loader's
                      torch.where(mask, x.flip(-1), x) for a seeded per-picture mask
               flip   decode_view_float(flip=mask)
  crop + flip  copy   decode_view_crop of 1/16 of the area at origins of their own, then the same torch.where
               flip   decode_view_crop(flip=mask)
and, once, the mirrored source: encode_view(flip="x") against torch.flip(x, [columns]) then encode_view.
Workloads: 64 gray frames of 4096 x 4096 and 256 RGB frames of 1920 x 1080 for the encodes (uint8), the RGB frames for the
decodes.  One process; every leg is warmed up, then the two legs of a pair take turns `reps` times and every call is timed
with HIP events around it.  Per leg the peak of torch's allocations above what the legs share is recorded too, and every
flipped leg's result is compared with its copy leg's, bit for bit.  The copy legs make only calls that need no flip keyword:
with "copy" as the last argument only they run, which is how the tool runs on a build without the keyword.
Under every pair the tool states the pair's condition itself: the flipped leg's median below the copy leg's median by more than
the copy leg's own spread (max - min over its reps) — met, or NOT met with the numbers.
Prints the table and, with an argument, writes it there too ("-": nowhere); "append" adds it to the file instead of
replacing it, under a line that says which legs ran: how profiles/flip_timing.txt takes the copy legs of another build.
usage: time_flip.py [out.txt [reps [small] [copy] [append]]]   (small: a few small frames, to try the tool out)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
small = "small" in sys.argv[3:]
copy_only = "copy" in sys.argv[3:]
append = "append" in sys.argv[3:]
ctx = dwt_amd.Context(0)
dev = ctx.device
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE, BIAS = tuple(1.0 / (255.0 * s) for s in STD), tuple(-m / s for m, s in zip(MEAN, STD))


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def same_streams(a, b):
    (oa, ia), (ob, ib) = a, b
    lens = ctx.stream_lengths(ia)
    live = torch.arange(oa.shape[1], device=dev)[None, :] < lens[:, None]
    return torch.equal(ia, ib) and torch.equal(oa * live, ob * live)


def pair(name, what, legs, same, rows):
    """legs: [(leg, fn)] with fn() -> the result; the copy leg first"""
    legs = legs[:1] if copy_only else legs
    peak, ref = {}, None
    for k, fn in legs:   # warm-up, then one call for the peak and the comparison
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        got = fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated(dev) - before) / 2**20
        if ref is None:
            ref = got
        else:
            assert same(ref, got), f"{name} {what} {k}: differs from the copy leg"
        del got
    del ref
    torch.cuda.empty_cache()
    ms = {k: [] for k, _ in legs}
    for _ in range(reps):
        for k, fn in legs:
            ms[k].append(timed(fn))
    base = sorted(ms[legs[0][0]])
    for k, _ in legs:
        v = sorted(ms[k])
        rows.append("%-18s %-12s %-5s %9.3f %8.3f %8.3f %7.3f %10.1f" % (name, what, k, v[len(v) // 2], v[0], v[-1], v[len(v) // 2] / base[len(base) // 2], peak[k]))
    if len(legs) == 2:
        flip, copy, spread = sorted(ms[legs[1][0]])[reps // 2], base[len(base) // 2], base[-1] - base[0]
        rows.append("    condition: flip %.3f %s copy %.3f - spread %.3f = %.3f: %s" % (flip, "<" if flip < copy - spread else ">=", copy, spread, copy - spread,
                                                                                 "met" if flip < copy - spread else "NOT met"))


def encodes(name, n, H, W, Cn, rows):
    upright = ctx.synth_pixels(n, H, W, Cn, 11, 0)
    for what, axis, key in (("encode y", 1, "y"), ("encode x", 2, "x")):
        lying = upright.flip(axis).contiguous()   # the batch as the caller has it: bottom-up, or mirrored
        pair(name, what, [("copy", lambda: ctx.encode_view(torch.flip(lying, [axis]))), ("flip", lambda: ctx.encode_view(lying, flip=key))], same_streams, rows)
        del lying
    torch.cuda.empty_cache()


def decodes(name, n, H, W, rows):
    pix = ctx.synth_pixels(n, H, W, 3, 11, 0)
    streams, info = ctx.encode_device(pix)
    lens = ctx.stream_lengths(info).clone()
    stride = (int(lens.max().item()) + 64 + 7) // 8 * 8
    streams = streams[:, :stride].contiguous()
    ctx.sync()
    del pix, info
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(n, generator=g) < 0.5
    dmask, flags = mask.to(dev)[:, None, None, None], [1 if m else 0 for m in mask.tolist()]
    cw, ch = W // 4, H // 4
    origins = [(int(x), int(y)) for x, y in zip(torch.randint(0, W - cw + 1, (n,), generator=g).tolist(), torch.randint(0, H - ch + 1, (n,), generator=g).tolist())]
    bits = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))   # noqa: E731

    def whole(flip):
        x = torch.empty((n, 3, H, W), dtype=torch.float16, device=dev)
        ctx.decode_view_float(streams, lens, x.permute(0, 2, 3, 1), scale=SCALE, bias=BIAS, **({"flip": flags} if flip else {}))
        return x if flip else torch.where(dmask, x.flip(-1), x)

    def crop(flip):
        x = torch.empty((n, 3, ch, cw), dtype=torch.float16, device=dev)
        ctx.decode_view_crop(streams, lens, x.permute(0, 2, 3, 1), (W, H), origins, scale=SCALE, bias=BIAS, **({"flip": flags} if flip else {}))
        return x if flip else torch.where(dmask, x.flip(-1), x)

    pair(name, "decode", [("copy", lambda: whole(False)), ("flip", lambda: whole(True))], bits, rows)
    pair(name, "crop + flip", [("copy", lambda: crop(False)), ("flip", lambda: crop(True))], bits, rows)
    torch.cuda.empty_cache()


lines = ["workload           call         leg   median ms   min ms   max ms   /copy   peak MiB of torch allocations",
         "-" * 104]
gray, rgb = ("64 x 4096^2 gray", 64, 4096, 4096, 1), ("256 x 1080p RGB", 256, 1080, 1920, 3)
if small:
    gray, rgb = ("4 x 520x264 gray", 4, 264, 520, 1), ("4 x 264x136 RGB", 4, 136, 264, 3)
rows = []
encodes(*gray, rows)
encodes(*rgb, rows)
decodes(rgb[0], rgb[1], rgb[2], rgb[3], rows)
text = "\n".join(lines + rows + ["reps %d, the two legs of a pair alternating, HIP events around each call; /copy: median over the median of the pair's copy leg%s"
                                 % (reps, "; copy legs only" if copy_only else "")])
print(text)
if out_path and out_path != "-":
    with open(out_path, "a" if append else "w") as f:
        if append:
            f.write("\n%s, in another run of tools/time_flip.py:\n" % ("the copy legs alone" if copy_only else "all legs"))
        f.write(text + "\n")
