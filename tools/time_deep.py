"""A deep workload, timed (development aid): 16 gray frames of 4096 x 4096, uint16 samples with maxval
4095, through encode_device16 and decode_device16 — 10 repeats, the two calls alternating, HIP events, medians with min and
max.  It uses nothing newer than the deep entry points, so the same file runs at an earlier commit: a change that must leave
the deep pictures' kernels alone is shown by running it at the parent commit and at the change in one session, which is how
the "deep workload" lines of profiles/signed_timing.txt were written (their first word is the label given here).
usage: time_deep.py [label]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

label = sys.argv[1] if len(sys.argv) > 1 else "this"
ctx = dwt_amd.Context(0)
n, H, W, C = 16, 4096, 4096, 1
pix = ctx.synth_pixels(n, H, W, C, 11, 0)
g = torch.Generator(device=ctx.device).manual_seed(11)
x = (pix.to(torch.int32) * 16 + torch.randint(0, 16, pix.shape, device=ctx.device, generator=g, dtype=torch.int32)).to(torch.int16)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


out, info = ctx.encode_device16(x)
lens = ctx.stream_lengths(info)
back, _ = ctx.decode_device16(out, lens, W, H, C, 4095)
assert torch.equal(back.view(torch.int16).view(x.shape), x)
enc = lambda: ctx.encode_device16(x, out=out, info=info)   # noqa: E731
dec = lambda: ctx.decode_device16(out, lens, W, H, C, 4095, out=back)   # noqa: E731
for fn in (enc, dec):
    fn()
    fn()
te, td = [], []
for _ in range(10):
    te.append(timed(enc))
    td.append(timed(dec))
te.sort()
td.sort()
print("%s: 16 x 4096x4096 gray uint16 (maxval 4095): encode_device16 median %.3f ms (min %.3f, max %.3f), decode_device16 median %.3f ms (min %.3f, max %.3f)"
      % (label, te[5], te[0], te[-1], td[5], td[0], td[-1]))
