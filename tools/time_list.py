"""Window lists against stack-then-call (development aid):
  encode  stack   what a caller with n separately allocated pictures does without dwtx_encode_view_list: torch.stack, then
                  encode_view (encode_view_float for the float pictures) of the stack
          list    encode_view_list of the n tensors where they lie
  decode  stack   decode_view (decode_view_float) into a new stack, then one copy_ per picture into the n tensors
          list    decode_view_list into the n tensors
  grid            the same windows as ONE tensor through encode_view / decode_view ...
  grid list       ... and spelled out as a list, n slices of that tensor: what the table look-up costs
Two workloads — 64 gray frames of 4096 x 4096 and 256 RGB frames of 1920 x 1080 — in uint8 (channel-last) and float16
(the RGB frames channel-first, as a model's tensors lie).  One process; every leg is warmed up, then the legs of a direction
take turns `reps` times and every call is timed with HIP events around it (the decodes end in the decoder's own
synchronisation, the encodes in the events').  Per leg the peak of torch's allocations above what the legs share (the n
tensors, the streams) is recorded too.  Every leg's result is compared with its partner's, bit for bit.
Prints a table and, with an argument, writes it there too ("-": nowhere).
usage: time_list.py [out.txt [reps [small]]]   (small: a few small frames, to try the tool out)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import dwt_amd

out_path = sys.argv[1] if len(sys.argv) > 1 else None
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
small = len(sys.argv) > 3 and sys.argv[3] == "small"
ctx = dwt_amd.Context(0)
dev = ctx.device
SCALE, BIAS = 1.0 / 255.0, -0.5        # the floats of a picture: x / 255 - 0.5
QUANT = dict(scale=255.0, bias=127.5)  # and back: rint(f * 255 + 127.5)


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


def workload(name, n, H, W, Cn, seed):
    rows = []
    pix = ctx.synth_pixels(n, H, W, Cn, seed, 0)
    for dtype in (torch.uint8, torch.float16):
        floats = dtype != torch.uint8
        bits = torch.int16 if floats else torch.uint8
        chw = floats and Cn == 3
        enc_more = QUANT if floats else {}
        dec_more = dict(scale=SCALE, bias=BIAS) if floats else {}

        def window(t):   # a tensor of a picture as the calls take it: [H,W,C]
            return t.permute(1, 2, 0) if chw else t

        def batch(t):
            return t.permute(0, 2, 3, 1) if chw else t

        shape = (Cn, H, W) if chw else (H, W, Cn)
        # n allocations of their own, in an order of the allocator's choosing, with the pictures in them
        sep = [torch.empty(shape, dtype=dtype, device=dev) for _ in range(n)]
        for i, t in enumerate(sep):
            p = pix[i].permute(2, 0, 1) if chw else pix[i]
            t.copy_((p.float() * SCALE + BIAS).to(dtype) if floats else p)
        one = torch.stack(sep)   # the same pictures as one tensor, for the grid legs
        encode_grid = ctx.encode_view_float if floats else ctx.encode_view
        decode_grid = ctx.decode_view_float if floats else ctx.decode_view
        streams, info = encode_grid(batch(one), **enc_more)
        lens = ctx.stream_lengths(info).clone()
        stride = (int(lens.max().item()) + 64 + 7) // 8 * 8
        streams = streams[:, :stride].contiguous()
        ctx.sync()
        # the lists themselves are made once: a caller that has n tensors has them as a list
        sep_w, one_w = [window(t) for t in sep], [window(one[i]) for i in range(n)]
        kept = {}

        def enc_stack():
            kept["e"] = encode_grid(batch(torch.stack(sep)), **enc_more)

        def enc_list():
            kept["e"] = ctx.encode_view_list(sep_w, **enc_more)

        def enc_grid():
            kept["e"] = encode_grid(batch(one), **enc_more)

        def enc_grid_list():
            kept["e"] = ctx.encode_view_list(one_w, **enc_more)

        def dec_stack():
            full = torch.empty((n,) + shape, dtype=dtype, device=dev)
            decode_grid(streams, lens, batch(full), **dec_more)
            for i, t in enumerate(sep):
                t.copy_(full[i])
            kept["d"] = sep

        def dec_list():
            ctx.decode_view_list(streams, lens, sep_w, **dec_more)
            kept["d"] = sep

        def dec_grid():
            decode_grid(streams, lens, batch(one), **dec_more)
            kept["d"] = [one]

        def dec_grid_list():
            ctx.decode_view_list(streams, lens, one_w, **dec_more)
            kept["d"] = [one]

        groups = [("encode", [("stack", enc_stack), ("list", enc_list)]), ("encode", [("grid", enc_grid), ("grid list", enc_grid_list)]),
                  ("decode", [("stack", dec_stack), ("list", dec_list)]), ("decode", [("grid", dec_grid), ("grid list", dec_grid_list)])]
        for direction, legs in groups:
            peak, ref = {}, None
            for k, fn in legs:   # warm-up (scratch, code objects, torch's allocator), then one call for the peak and the comparison
                fn()
                kept.clear()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                if direction == "decode":
                    for t in sep + [one]:
                        t.zero_()
                fn()
                torch.cuda.synchronize()
                peak[k] = (torch.cuda.max_memory_allocated(dev) - before) / 2**20
                got = kept["e"] if direction == "encode" else torch.stack([t.view(bits) for t in kept["d"]]).reshape(-1).clone()
                if ref is None:
                    ref = got
                elif direction == "encode":
                    assert same_streams(ref, got), f"{name} {dtype} encode {k}: differs from its partner"
                else:
                    assert torch.equal(ref, got), f"{name} {dtype} decode {k}: differs from its partner"
                kept.clear()
                del got
            del ref
            torch.cuda.empty_cache()
            ms = {k: [] for k, _ in legs}
            for _ in range(reps):
                for k, fn in legs:
                    ms[k].append(timed(fn))
                    kept.clear()
            base = sorted(ms[legs[0][0]])
            for k, _ in legs:
                v = sorted(ms[k])
                rows.append("%-18s %-8s %-7s %-10s %9.3f %8.3f %8.3f %7.3f %10.1f" % (
                    name, str(dtype).replace("torch.", ""), direction, k, v[len(v) // 2], v[0], v[-1], v[len(v) // 2] / base[len(base) // 2], peak[k]))
        del sep, one, sep_w, one_w, streams, info
        torch.cuda.empty_cache()
    return rows


lines = ["workload           samples  call    leg         median ms   min ms   max ms   /first   peak MiB of torch allocations",
         "-" * 112]
loads = [("64 x 4096^2 gray", 64, 4096, 4096, 1), ("256 x 1080p RGB", 256, 1080, 1920, 3)]
if small:
    loads = [("4 x 520x264 gray", 4, 264, 520, 1), ("4 x 264x136 RGB", 4, 136, 264, 3)]
for name, n, H, W, Cn in loads:
    lines += workload(name, n, H, W, Cn, 11)
text = "\n".join(lines + ["reps %d, the two legs of a pair alternating, HIP events around each call; /first: median over the median of the pair's first leg" % reps])
print(text)
if out_path and out_path != "-":
    with open(out_path, "w") as f:
        f.write(text + "\n")
