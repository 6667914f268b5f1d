"""Clip stacks against what a caller writes without them (development aid).  Per workload, these legs:
  decode  clips    decode_view_clips(streams, lens, back, period)
          pairs    per clip one plain decode_view of the key's stream and one decode_view_chain of the clip's links, the key as key
  encode  clips    encode_view_clips(t, period)
          pairs    per clip one plain encode_view of the key and one encode_view(t[k+1:e], base=t[k:e-1]) of its links
          delta    ONE encode_view(t[1:], base=t[:-1]) of n - 1 pictures: other streams (no keys), but the same pipeline behind the
                   wide finest-level sources of section 4.21 where the layout has them — what the clips call gives up by going
                   through the general conversion.  Reported, not bounded.
and, on one stack of workload 2's slices, the segment dimension: decode_view_clips with period = n against the pair it replaces,
a plain decode of the key and ONE decode_view_chain of the n - 1 links — the same chain, walked by k_clips_from_planes with one
segment and by k_chain_from_planes.
Workloads: 64 clips of 16 frames of 224 x 224 RGB uint8 (n = 1024, period 16), 8 volumes of 64 slices of 512 x 512 int16 in
[-1024, 3071] (n = 512, period 64) and 64 frames of 1920 x 1080 RGB uint8 with period 8; frame i is the synthetic frame of seed
i (the same scene, other noise).
One process; each leg is warmed up, then the legs take turns `reps` times.  Every leg is timed with the host's clock from a
synchronised device to a final synchronise: the pairs' cost is their host round trips, which device events around single calls
would not show.  Results are asserted: every decode leg gives the frames back, the pairs' streams are the clips call's.  Prints
a table and, with an argument, writes it there too ("-": nowhere).
usage: time_clips.py [out.txt [reps [workload index]]]"""
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def frames(n, H, W, Cn, lo, hi):
    """[n,H,W,C] in [lo, hi]: the synthetic 8-bit frames of seeds 0 .. n - 1 — uint8 as they are, or stretched over an int16
    range with the bits below filled with noise (tools/time_chain.py)"""
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


def workload(n, H, W, Cn, lo, hi, period):
    sgn = lo < 0
    t = frames(n, H, W, Cn, lo, hi)
    spans = [(k, min(k + period, n)) for k in range(0, n, period)]
    out, info = ctx.encode_view_clips(t, period, signed=sgn)
    lens = ctx.stream_lengths(info)
    bufs = (torch.empty_like(out), torch.empty_like(info))

    def enc_clips():
        ctx.encode_view_clips(t, period, out=bufs[0], info=bufs[1], signed=sgn)

    def enc_pairs():
        for k, e in spans:
            ctx.encode_view(t[k:k + 1], out=bufs[0][k:k + 1], info=bufs[1][k:k + 1], signed=sgn)
            if e > k + 1:
                ctx.encode_view(t[k + 1:e], out=bufs[0][k + 1:e], info=bufs[1][k + 1:e], signed=sgn, base=t[k:e - 1])

    enc_pairs()
    lens2 = ctx.stream_lengths(bufs[1])
    assert torch.equal(lens, lens2), "the pairs' streams are not the clips call's"
    assert all(torch.equal(out[i, :int(lens[i])], bufs[0][i, :int(lens[i])]) for i in range(0, n, 5)), "the pairs' streams are not the clips call's"
    wide = (torch.empty_like(out[1:]), torch.empty_like(info[1:]))
    enc = measure({"clips": enc_clips, "pairs": enc_pairs,
                   "delta": lambda: ctx.encode_view(t[1:], out=wide[0], info=wide[1], signed=sgn, base=t[:-1])})
    kw = dict(maxval=hi, signed=sgn, minval=lo if sgn else None)
    back = torch.zeros_like(t)

    def dec_clips():
        ctx.decode_view_clips(out, lens, back, period, **kw)

    def dec_pairs():
        for k, e in spans:
            ctx.decode_view(out[k:k + 1], lens[k:k + 1], back[k:k + 1], **kw)
            if e > k + 1:
                ctx.decode_view_chain(out[k + 1:e], lens[k + 1:e], back[k + 1:e], back[k], **kw)

    for name, fn in (("clips", dec_clips), ("pairs", dec_pairs)):
        back.zero_()
        fn()
        assert torch.equal(back, t), f"the {name} leg does not give the frames back"
    dec = measure({"clips": dec_clips, "pairs": dec_pairs})
    return enc, dec, int(lens.sum())


def one_stack(n, H, W, Cn, lo, hi):
    """period = n: one chain with its key inside the stack, against the key's plain decode and the chain call on the rest"""
    sgn = lo < 0
    t = frames(n, H, W, Cn, lo, hi)
    out, info = ctx.encode_view_clips(t, n, signed=sgn)
    lens = ctx.stream_lengths(info)
    kw = dict(maxval=hi, signed=sgn, minval=lo if sgn else None)
    back = torch.zeros_like(t)

    def clips():
        ctx.decode_view_clips(out, lens, back, n, **kw)

    def pair():
        ctx.decode_view(out[:1], lens[:1], back[:1], **kw)
        ctx.decode_view_chain(out[1:], lens[1:], back[1:], back[0], **kw)

    for name, fn in (("clips", clips), ("pair", pair)):
        back.zero_()
        fn()
        assert torch.equal(back, t), f"the {name} leg does not give the frames back"
    return measure({"clips": clips, "pair": pair})


def spread(r):
    return r[2] - r[1]


WORKLOADS = (("64 clips x 16 x 224x224 RGB uint8", (1024, 224, 224, 3, 0, 255, 16)), ("8 volumes x 64 x 512x512 int16", (512, 512, 512, 1, -1024, 3071, 64)),
             ("64 x 1080p RGB uint8, period 8", (64, 1080, 1920, 3, 0, 255, 8)))
lines = ["workload                            call     leg       median ms   min ms   max ms", "-" * 84]
for k, (name, args) in enumerate(WORKLOADS):
    if only >= 0 and k != only:
        continue
    enc, dec, nbytes = workload(*args)
    torch.cuda.empty_cache()
    for call, rows in (("encode", enc), ("decode", dec)):
        for leg, r in rows.items():
            lines.append("%-35s %-8s %-9s %9.3f %8.3f %8.3f" % (name, call, leg, r[0], r[1], r[2]))
    for call, rows in (("encode", enc), ("decode", dec)):
        c, p = rows["clips"], rows["pairs"]
        lines.append("%-35s %-8s clips / pairs: %.3f of the time (medians); pairs - clips: %.3f ms; spread of the repeats: clips %.3f ms, "
                     "pairs %.3f ms; clips below pairs by more than both spreads: %s" %
                     (name, call, c[0] / p[0], p[0] - c[0], spread(c), spread(p), "yes" if p[0] - c[0] > spread(c) + spread(p) else "NO"))
    lines.append("%-35s encode   clips / delta (n - 1 links, no keys, wide sources where the layout has them): %.3f" % (name, enc["clips"][0] / enc["delta"][0]))
    lines.append("%-35s stream bytes: %d" % (name, nbytes))
if only < 0 or only == len(WORKLOADS):
    name = "1 stack x 64 x 512x512 int16"
    r = one_stack(64, 512, 512, 1, -1024, 3071)
    for leg, v in r.items():
        lines.append("%-35s %-8s %-9s %9.3f %8.3f %8.3f" % (name, "decode", leg, v[0], v[1], v[2]))
    c, p = r["clips"], r["pair"]
    lines.append("%-35s decode   segment dimension, period = n: clips / pair: %.3f of the time (medians); clips - pair: %.3f ms; spread of the "
                 "repeats: clips %.3f ms, pair %.3f ms; clips costs the single chain more than the two legs' spread: %s" %
                 (name, c[0] / p[0], c[0] - p[0], spread(c), spread(p), "YES" if c[0] - p[0] > spread(c) + spread(p) else "no"))
text = "\n".join(lines + ["reps %d, legs alternating, host clock from a synchronised device to a final synchronise; decoded samples and streams asserted equal" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
