"""Delta chains, three decode legs (development aid):
  chain    the chain call: decode_view_chain(streams, lens, back[1:], back[0])
  loop     what a caller had to write before it: n calls of decode_view(streams[i:i+1], ..., back[i+1:i+2], base=back[i:i+1])
  delta    the same streams in one plain delta decode onto an INDEPENDENT base (the true frames 0 .. n-1): no chain, and so the
           fused sinks — what giving those up costs the chain call.  Reported, not bounded.
and the encode beside them: encode_view_chain(t[1:], t[0]) against encode_view(t[1:], base=t[:-1]), which is one call already.
Workloads: 64 gray frames of 4096 x 4096 uint8, 256 gray slices of 512 x 512 int16 in [-1024, 3071] (a CT volume) and 64 frames
of 1920 x 1080 RGB uint8; frame i is the synthetic frame of seed i (the same scene, other noise), frame 0 the key.
One process; each leg is warmed up, then the legs take turns `reps` times.  Every leg is timed with the host's clock from a
synchronised device to a final synchronise: the loop's cost is its n host round trips, which device events around single
calls would not show.  The decodes' results are asserted: every leg gives the frames back.  Prints a table and, with an
argument, writes it there too ("-": nowhere).
usage: time_chain.py [out.txt [reps [workload index]]]"""
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
    range with the bits below filled with noise (tools/time_delta.py)"""
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


def workload(n, H, W, Cn, lo, hi):
    sgn = lo < 0
    t = frames(n + 1, H, W, Cn, lo, hi)
    out, info = ctx.encode_view_chain(t[1:], t[0], signed=sgn)
    out2, info2 = ctx.encode_view(t[1:], signed=sgn, base=t[:-1])
    lens = ctx.stream_lengths(info)
    assert torch.equal(lens, ctx.stream_lengths(info2)), "the chain encode's streams are not the delta call's"
    assert all(torch.equal(out[i, :int(lens[i])], out2[i, :int(lens[i])]) for i in range(0, n, 7)), "the chain encode's streams are not the delta call's"
    bufs = (torch.empty_like(out), torch.empty_like(info))
    enc = measure({
        "chain": lambda: ctx.encode_view_chain(t[1:], t[0], out=bufs[0], info=bufs[1], signed=sgn),
        "delta": lambda: ctx.encode_view(t[1:], out=bufs[0], info=bufs[1], signed=sgn, base=t[:-1])})
    kw = dict(maxval=hi, signed=sgn, minval=lo if sgn else None)
    back = torch.zeros_like(t)
    back[0] = t[0]
    into = torch.zeros_like(t[1:])

    def chain():
        ctx.decode_view_chain(out, lens, back[1:], back[0], **kw)

    def loop():
        for i in range(n):
            ctx.decode_view(out[i:i + 1], lens[i:i + 1], back[i + 1:i + 2], base=back[i:i + 1], **kw)

    def delta():
        ctx.decode_view(out, lens, into, base=t[:-1], **kw)

    for name, fn, res in (("chain", chain, back), ("loop", loop, back), ("delta", delta, None)):
        back[1:] = 0
        fn()
        assert torch.equal(back, t) if res is back else torch.equal(into, t[1:]), f"the {name} leg does not give the frames back"
    dec = measure({"chain": chain, "loop": loop, "delta": delta})
    return enc, dec, int(lens.sum())


WORKLOADS = (("64 x 4096x4096 gray uint8", (64, 4096, 4096, 1, 0, 255)), ("256 x 512x512 gray int16", (256, 512, 512, 1, -1024, 3071)),
             ("64 x 1080p RGB uint8", (64, 1080, 1920, 3, 0, 255)))
lines = ["workload                        call     leg       median ms   min ms   max ms", "-" * 80]
for k, (name, args) in enumerate(WORKLOADS):
    if only >= 0 and k != only:
        continue
    enc, dec, nbytes = workload(*args)
    torch.cuda.empty_cache()
    for call, rows in (("encode", enc), ("decode", dec)):
        for leg, r in rows.items():
            lines.append("%-31s %-8s %-9s %9.3f %8.3f %8.3f" % (name, call, leg, r[0], r[1], r[2]))
    c, d = enc["chain"], enc["delta"]
    lines.append("%-31s encode   chain / delta: %.3f of the time (medians); spread of the repeats: chain %.3f ms, delta %.3f ms" %
                 (name, c[0] / d[0], c[2] - c[1], d[2] - d[1]))
    c, l, d = dec["chain"], dec["loop"], dec["delta"]
    lines.append("%-31s decode   chain / loop: %.3f, chain / delta: %.3f of the time (medians); loop - chain: %.3f ms; spread of the repeats: "
                 "chain %.3f ms, loop %.3f ms, delta %.3f ms; chain below loop by more than both spreads: %s" %
                 (name, c[0] / l[0], c[0] / d[0], l[0] - c[0], c[2] - c[1], l[2] - l[1], d[2] - d[1],
                  "yes" if l[0] - c[0] > (c[2] - c[1]) + (l[2] - l[1]) else "NO"))
    lines.append("%-31s stream bytes: %d" % (name, nbytes))
text = "\n".join(lines + ["reps %d, legs alternating, host clock from a synchronised device to a final synchronise; decoded samples asserted equal" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
