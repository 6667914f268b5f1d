"""GPU: the buffer bounds of include/dwtx.h.

Every other decode test hands the decoder streams followed by zeros, which hides a read past a stream's length that is
not masked: zero bits decode as more empty data.  Here each stream is followed by live bytes (the rest of the uncut
stream, 0xff, noise, another stream), and the last stream of a batch can end exactly where the batch ends.  The write
side is pinned the same way: streams into strides shorter than themselves, pictures into padded or misaligned pixel
buffers, a packed message into a short buffer.

Every buffer a test hands to the library is a view into a larger one the test owns, with a guard of at least 4 KiB
behind the last slot: a stray access lands in the test's memory and shows up as a changed result or a changed guard
byte.  No call gets less memory than include/dwtx.h asks for."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

GUARD = 4096
FILLS = ("zero", "continuation", "ones", "random", "foreign")
ERR_CAPACITY, ERR_ARG = -2, -3


def _r4(v):
    return (v + 3) // 4 * 4


def _r8(v):
    return (v + 7) // 8 * 8


def _canary(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


# ---- stream layouts ----------------------------------------------------------------------------------------------

def layout(fulls, cuts, fill, stride, seed=0):
    """Row i of an [n, stride] batch holds fulls[i][:cuts[i]] followed by `fill`; behind the n rows a noise tail of GUARD
    bytes.  Returns the whole host buffer (n * stride + GUARD bytes).
      zero          today's layout
      continuation  the rest of the uncut stream (a prefix decode from the full stream's buffer), then noise
      ones          0xff
      random        noise
      foreign       another stream's bytes, from its start (what a `rows` gather leaves behind)"""
    n = len(fulls)
    big = _canary(n * stride + GUARD, 1000 + seed)
    rows = big[:n * stride].reshape(n, stride)
    for i, (full, cut) in enumerate(zip(fulls, cuts)):
        a = np.frombuffer(full, dtype=np.uint8)
        cut = min(cut, stride)
        rows[i, :cut] = a[:cut]
        rest = rows[i, cut:]
        if fill == "zero":
            rest[:] = 0
        elif fill == "ones":
            rest[:] = 255
        elif fill == "continuation":
            k = min(len(a) - cut, rest.size)
            rest[:k] = a[cut:cut + k]
        elif fill == "foreign":
            other = np.frombuffer(fulls[(i + 1) % n], dtype=np.uint8)
            if rest.size:
                rest[:] = np.resize(other, rest.size)
        else:
            assert fill == "random"
    return big


class Oracle:
    """orc.decode_stage / orc.decode of stream prefixes, each computed once."""

    def __init__(self, W, H, Cn):
        self.W, self.H, self.Cn = W, H, Cn
        self.stage_memo, self.pix_memo = {}, {}

    def stage(self, data, pixels_max=-1):
        key = (data, pixels_max)
        if key not in self.stage_memo:
            self.stage_memo[key] = orc.decode_stage(data, self.W, self.H, self.Cn, pixels_max)
        return self.stage_memo[key]

    def pixels(self, data, pixels_max=-1):
        key = (data, pixels_max)
        if key not in self.pix_memo:
            self.pix_memo[key] = orc.decode(data, pixels_max)
        return self.pix_memo[key]


def _levels_max(W, H, pixels_max):
    if pixels_max < 0:
        return -1
    g = orc.geometry(W, H)
    lm = g.levels
    while lm > 0 and g.pixels[lm] > pixels_max:
        lm -= 1
    return lm


# ---- the three decode entry points on a laid-out batch ------------------------------------------------------------

def decode_planes(ctx, big, stride, lens, W, H, Cn, levels_max=-1):
    """dwtx_decode_planes on the rows of `big`: -> (lin int32 [n, C, W*H], infos)."""
    import torch

    import dwt_amd

    n = len(lens)
    dev = torch.from_numpy(big).to(ctx.device)
    dl = torch.tensor(lens, dtype=torch.int64, device=ctx.device)
    lin = torch.empty((n * Cn, W * H), dtype=torch.int32, device=ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()
    rc = ctx.lib.dwtx_decode_planes(ctx.h, lin.data_ptr(), dev.data_ptr(), stride, dl.data_ptr(), W, H, Cn, n, levels_max,
                                    C.cast(infos, C.c_void_p))
    assert rc == 0, ctx.lib.dwtx_last_error()
    got = lin.cpu().numpy().reshape(n, Cn, W * H)
    assert (dev.cpu().numpy() == big).all()   # const input
    return got, list(infos)


def check_planes(orcl, fulls, cuts, got, infos, pixels_max=-1):
    for i, (full, cut) in enumerate(zip(fulls, cuts)):
        ref = orcl.stage(full[:cut], pixels_max)
        where = f"row {i}, {cut} of {len(full)} bytes"
        if ref is None:
            assert infos[i].status == 1, where
            continue
        rlin, level, missing, planes = ref
        assert infos[i].status == 0, where
        assert list(infos[i].planes)[:orcl.Cn] == planes, where
        assert infos[i].level == level, where
        assert list(infos[i].missing) == missing.tolist(), where
        assert (got[i] == rlin).all(), where


def decode_device(ctx, big, stride, lens, W, H, Cn, levels_max=-1, pix_stride=None, pix_off=0, expect=0):
    """dwtx_decode_device on the rows of `big` into a guarded pixel buffer: picture i at pix_off + i * pix_stride.
    -> (infos, pixel buffer after the call, pixel buffer before it)."""
    import torch

    import dwt_amd

    n = len(lens)
    if pix_stride is None:
        pix_stride = W * H * Cn
    dev = torch.from_numpy(big).to(ctx.device)
    dl = torch.tensor(lens, dtype=torch.int64, device=ctx.device)
    before = _canary(pix_off + n * pix_stride + GUARD, 77 + n + pix_off)
    out = torch.from_numpy(before).to(ctx.device)
    infos = (dwt_amd.DecodeInfo * n)()
    rc = ctx.lib.dwtx_decode_device(ctx.h, dev.data_ptr(), stride, dl.data_ptr(), W, H, Cn, n, levels_max,
                                    out.data_ptr() + pix_off, pix_stride, C.cast(infos, C.c_void_p))
    assert rc == expect, (rc, ctx.lib.dwtx_last_error())
    after = out.cpu().numpy()
    assert (dev.cpu().numpy() == big).all()
    return list(infos), after, before


def check_pixels(orcl, fulls, cuts, infos, after, before, pix_stride, pix_off=0, pixels_max=-1, sizes=None):
    """Picture i equals the oracle's decode of fulls[i][:cuts[i]]; every other byte of the buffer is as it was."""
    want_buf = before.copy()
    for i, (full, cut) in enumerate(zip(fulls, cuts)):
        ref = orcl.pixels(full[:cut], pixels_max)
        where = f"row {i}, {cut} of {len(full)} bytes"
        if infos is not None:
            assert (infos[i].status == 0) == (ref is not None), where
        if sizes is not None:
            assert sizes[i] == ((ref.shape[1], ref.shape[0], ref.shape[2]) if ref is not None else (0, 0)), where
        if ref is None:
            continue
        o = pix_off + i * pix_stride
        assert (after[o:o + ref.size] == ref.reshape(-1)).all(), where
        want_buf[o:o + ref.size] = ref.reshape(-1)
    bad = np.nonzero(after != want_buf)[0]
    assert bad.size == 0, f"{bad.size} bytes outside the pictures changed, first at {bad[0]} (pix_stride {pix_stride})"


INFO_FIELDS = ("status", "level", "nsegs", "truncated", "pmax", "bits_used", "zeros_left")


def same_infos(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        for f in INFO_FIELDS:
            assert getattr(x, f) == getattr(y, f), (what, i, f)
        assert list(x.planes) == list(y.planes) and list(x.missing) == list(y.missing), (what, i)


def decode_images(ctx, big, stride, lens, W, H, Cn, pixels_max=-1, pix_stride=None, pix_off=0, expect=0):
    """dwtx_decode_images on host rows -> (sizes [(w, h, c)], pixel buffer after, before)."""
    n = len(lens)
    if pix_stride is None:
        pix_stride = W * H * Cn
    before = _canary(pix_off + n * pix_stride + GUARD, 99 + n + pix_off)
    after = before.copy()
    hl = (C.c_size_t * n)(*lens)
    ow, oh, oc = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    keep = big.copy()
    rc = ctx.lib.dwtx_decode_images(ctx.h, big.ctypes.data, stride, C.cast(hl, C.c_void_p), n, pixels_max,
                                    after.ctypes.data + pix_off, pix_stride, ow, oh, oc)
    assert rc == expect, (rc, ctx.lib.dwtx_last_error())
    assert (keep == big).all()
    return [(ow[i], oh[i], oc[i]) if ow[i] else (0, 0) for i in range(n)], after, before


# ---- streams and cut points ---------------------------------------------------------------------------------------

SHAPES = {   # (H, W, C): the decoder paths they reach
    "gray_w4": (150, 212, 1),     # W % 4 == 0 above 64 px: the fused u8 inverse
    "gray_square": (256, 256, 1),  # power-of-two square: the tile paths and the 16-bit finest rings
    "rgb": (97, 131, 3),
    "rgb_square": (128, 128, 3),
}


def streams_of(shape, k=4):
    H, W, Cn = shape
    out = []
    for s in range(k):
        data, st = orc.encode(orc.synth(W, H, Cn, 40 + s, s & 1))
        out.append((data, st))
    return out


def cut_points(data, st, rng):
    """Inside the header, the root image and the plane counts; at every residue mod 16 around a few 128-bit chunk
    boundaries; a dozen anywhere (refinement blocks are a large part of every stream); len - 1; the whole stream."""
    L = len(data)
    hdr = (st.meta_bits + st.root_bits) // 8
    cuts = {3, 5, 6, 7, 8, 9, 12}
    cuts |= set(range(max(1, hdr - 2), hdr + 4))
    for k in (2, 7, L // 32, L // 16 - 1):
        cuts |= set(range(16 * k - 8, 16 * k + 8))
    cuts |= set(int(v) for v in rng.integers(hdr, L, 12))
    cuts |= {L - 1, L}
    return sorted(c for c in cuts if 1 <= c <= L)


def batch_of(shape, seed=0):
    """(fulls, cuts, oracle) rows of the chunk-boundary batch of one shape: the full stream is first, so that the
    host entry point (which reads the geometry off row 0) sees a header."""
    H, W, Cn = shape
    rng = np.random.default_rng(seed)
    fulls, cuts = [], []
    for data, st in streams_of(shape):
        for c in cut_points(data, st, rng):
            fulls.append(data)
            cuts.append(c)
    order = sorted(range(len(cuts)), key=lambda i: cuts[i] != len(fulls[i]))   # whole streams first (stable)
    return [fulls[i] for i in order], [cuts[i] for i in order], Oracle(W, H, Cn)


_BATCHES = {}


def cached_batch(name):
    if name not in _BATCHES:
        _BATCHES[name] = batch_of(SHAPES[name], seed=len(_BATCHES))
    return _BATCHES[name]


# ---- 1. decoding with live bytes past each stream's length -------------------------------------------------------

@pytest.mark.parametrize("fill", ["continuation", "ones"])
def test_every_prefix_of_a_small_rgb_stream_with_live_bytes_behind_it(ctx, fill):
    """All byte prefixes of a 53x37 RGB stream, each row holding the whole stream (or the prefix and 0xff), through
    dwtx_decode_planes and dwtx_decode_device; the records equal those of the zero-filled batch."""
    W, H, Cn = 53, 37, 3
    data, _ = orc.encode(orc.synth(W, H, Cn, 5, 0))
    L = len(data)
    stride = _r8(L)
    orcl = Oracle(W, H, Cn)
    for first in range(1, L + 1, 1024):
        cuts = list(range(first, min(first + 1024, L + 1)))
        fulls = [data] * len(cuts)
        big = layout(fulls, cuts, fill, stride, seed=first)
        got, infos = decode_planes(ctx, big, stride, cuts, W, H, Cn)
        check_planes(orcl, fulls, cuts, got, infos)
        dinfos, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn)
        check_pixels(orcl, fulls, cuts, dinfos, after, before, W * H * Cn)
        zinfos, _, _ = decode_device(ctx, layout(fulls, cuts, "zero", stride, seed=first), stride, cuts, W, H, Cn)
        same_infos(dinfos, zinfos, fill)


@pytest.mark.parametrize("name", list(SHAPES))
def test_cuts_around_chunk_boundaries_under_every_fill(ctx, name, opts):
    """Four streams per shape, cut inside the header, root image and plane counts, at all 16 residues around 128-bit
    chunk boundaries, anywhere, at len - 1 and not at all; under every fill, through all three decode entry points.
    The host pipeline runs the batch in parts of 64 images."""
    H, W, Cn = SHAPES[name]
    fulls, cuts, orcl = cached_batch(name)
    stride = _r8(max(len(f) for f in fulls))   # the longest stream ends at its row's end, or within 7 bytes of it
    zinfos = zpinfos = None
    opts.set("part_images", 64)
    for fill in ("zero",) + tuple(f for f in FILLS if f != "zero"):
        big = layout(fulls, cuts, fill, stride, seed=len(fill))
        got, infos = decode_planes(ctx, big, stride, cuts, W, H, Cn)
        check_planes(orcl, fulls, cuts, got, infos)
        dinfos, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn)
        check_pixels(orcl, fulls, cuts, dinfos, after, before, W * H * Cn)
        if zinfos is None:
            zinfos, zpinfos = dinfos, infos
        same_infos(dinfos, zinfos, fill)
        same_infos(infos, zpinfos, fill)
        sizes, hafter, hbefore = decode_images(ctx, big, stride, cuts, W, H, Cn)
        check_pixels(orcl, fulls, cuts, None, hafter, hbefore, W * H * Cn, sizes=sizes)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_last_stream_ends_where_the_batch_ends(ctx, name):
    """The stride is a multiple of 8 no longer than the shortest stream: every row is full of stream bytes, the last
    one ends exactly at n * stride, and a noise tail follows the batch."""
    H, W, Cn = SHAPES[name]
    fulls = [d for d, _ in streams_of(SHAPES[name])]
    stride = min(len(f) for f in fulls) // 8 * 8
    orcl = Oracle(W, H, Cn)
    for cuts in ([stride] * 4, [stride - 9, stride - 1, stride - 16, stride]):
        big = layout(fulls, cuts, "continuation", stride, seed=cuts[0])
        got, infos = decode_planes(ctx, big, stride, cuts, W, H, Cn)
        check_planes(orcl, fulls, cuts, got, infos)
        dinfos, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn)
        check_pixels(orcl, fulls, cuts, dinfos, after, before, W * H * Cn)
        sizes, hafter, hbefore = decode_images(ctx, big, stride, cuts, W, H, Cn)
        check_pixels(orcl, fulls, cuts, None, hafter, hbefore, W * H * Cn, sizes=sizes)


@pytest.mark.parametrize("option", [("decode_parts", 2), ("decode_parts", 3), ("decode_parts", 4), ("two_families", 1),
                                    ("one_stream", 1)])
@pytest.mark.parametrize("name", ["rgb", "gray_square"])
def test_decoder_variants_with_live_bytes(ctx, name, option, opts):
    H, W, Cn = SHAPES[name]
    fulls, cuts, orcl = cached_batch(name)
    stride = _r8(max(len(f) for f in fulls))
    opts.set(*option)
    for fill in ("random", "continuation"):
        big = layout(fulls, cuts, fill, stride, seed=7)
        dinfos, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn)
        check_pixels(orcl, fulls, cuts, dinfos, after, before, W * H * Cn)


@pytest.mark.parametrize("pixels_max", [0, 300, 5000, 20000])
def test_pixels_cap_with_live_bytes(ctx, pixels_max):
    name = "rgb"
    H, W, Cn = SHAPES[name]
    fulls, cuts, orcl = cached_batch(name)
    stride = _r8(max(len(f) for f in fulls))
    big = layout(fulls, cuts, "ones", stride, seed=3)
    lm = _levels_max(W, H, pixels_max)
    got, infos = decode_planes(ctx, big, stride, cuts, W, H, Cn, levels_max=lm)
    check_planes(orcl, fulls, cuts, got, infos, pixels_max=pixels_max)
    dinfos, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn, levels_max=lm)
    check_pixels(orcl, fulls, cuts, dinfos, after, before, W * H * Cn, pixels_max=pixels_max)
    sizes, hafter, hbefore = decode_images(ctx, big, stride, cuts, W, H, Cn, pixels_max=pixels_max)
    check_pixels(orcl, fulls, cuts, None, hafter, hbefore, W * H * Cn, pixels_max=pixels_max, sizes=sizes)


@pytest.mark.parametrize("name", ["gray_square", "rgb"])
def test_the_full_streams_index_offered_for_its_prefixes(ctx, name):
    """The sidecar index of a whole stream, offered for prefixes of it that are followed by the rest of the stream or
    by noise: it may speed the decode up, the result is the oracle's on the prefix."""
    import dwt_amd

    H, W, Cn = SHAPES[name]
    fulls0 = [d for d, _ in streams_of(SHAPES[name])]
    stride = _r8(max(len(f) for f in fulls0))
    made = ctx.set_index(None, len(fulls0))
    try:
        decode_planes(ctx, layout(fulls0, [len(f) for f in fulls0], "zero", stride), stride, [len(f) for f in fulls0], W, H, Cn)
        assert all(m.nsegs > 0 for m in made)
        rng = np.random.default_rng(11)
        fulls, cuts, which = [], [], []
        for s, f in enumerate(fulls0):
            for c in sorted(set(int(v) for v in rng.integers(6, len(f), 24)) | {len(f) - 1, len(f) // 2}):
                fulls.append(f)
                cuts.append(c)
                which.append(s)
        offered = (dwt_amd.Index * len(fulls))(*[made[s] for s in which])
        orcl = Oracle(W, H, Cn)
        for fill in ("continuation", "random"):
            ctx.set_index(offered, 0)
            big = layout(fulls, cuts, fill, stride, seed=5)
            got, infos = decode_planes(ctx, big, stride, cuts, W, H, Cn)
            check_planes(orcl, fulls, cuts, got, infos)
            dinfos, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn)
            check_pixels(orcl, fulls, cuts, dinfos, after, before, W * H * Cn)
    finally:
        ctx.set_index()


# ---- 2. encoding into a stride shorter than the stream -----------------------------------------------------------

ENC_SHAPES = [(96, 128, 1), (37, 53, 3), (64, 64, 3)]


def _enc_pictures(shape, n=4):
    H, W, Cn = shape
    return np.stack([orc.synth(W, H, Cn, 60 + s, s & 1) for s in range(n)])


def _enc_strides(L, align):
    r = lambda v: (v + align - 1) // align * align   # noqa: E731
    return sorted({8, 12 if align == 4 else 16, max(8, r(L // 2)), r(L) - align, r(L), r(L) + align})


def expected_slots(streams, nbytes, stride, guard_seed, n):
    """The output buffer the contract allows: slot i holds the first min(stride, nbytes) bytes of stream i; a stream
    that ends inside its slot is followed by zeros up to min(stride, round4(nbytes) + 16); nothing else changes."""
    buf = _canary(n * stride + GUARD, guard_seed)
    for i in range(n):
        m = min(stride, nbytes[i])
        o = i * stride
        buf[o:o + m] = np.frombuffer(streams[i][:m], dtype=np.uint8)
        z = min(stride, _r4(nbytes[i]) + 16)
        if z > m:
            buf[o + m:o + z] = 0
    return buf


@pytest.mark.parametrize("entry", ["planes", "device"])
@pytest.mark.parametrize("shape", ENC_SHAPES)
def test_encode_into_strides_shorter_than_the_stream(ctx, entry, shape):
    """dwtx_encode_planes / dwtx_encode_device: slot i holds the oracle's stream up to the stride, zeros behind a
    stream that ends inside its slot (k_clear_stream's rule), and not a byte past the slot changes."""
    import torch

    import dwt_amd

    H, W, Cn = shape
    pix = _enc_pictures(shape)
    n = pix.shape[0]
    dpix = torch.from_numpy(pix).to(ctx.device)
    lin = None
    if entry == "planes":
        lin = torch.from_numpy(np.concatenate([orc.stage_dump(p)[1] for p in pix])).to(ctx.device)
    L = len(orc.encode(pix[1])[0])
    for stride in _enc_strides(L, 4):
        for capacity in (0, stride + 100):
            want = [orc.encode(p, capacity) for p in pix]
            seed = stride + capacity
            out = torch.from_numpy(_canary(n * stride + GUARD, seed)).to(ctx.device)
            info = torch.zeros((n, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
            if entry == "planes":
                rc = ctx.lib.dwtx_encode_planes(ctx.h, lin.data_ptr(), W, H, Cn, n, capacity, out.data_ptr(), stride, info.data_ptr())
            else:
                rc = ctx.lib.dwtx_encode_device(ctx.h, dpix.data_ptr(), W, H, Cn, n, capacity, out.data_ptr(), stride, info.data_ptr())
            assert rc == 0, ctx.lib.dwtx_last_error()
            raw = info.cpu().numpy()
            infos = [dwt_amd.StreamInfo.from_buffer_copy(raw[i].tobytes()) for i in range(n)]
            for i in range(n):
                assert infos[i].nbytes == len(want[i][0]), (stride, capacity, i)
                assert infos[i].total_bits == want[i][1].total_bits, (stride, capacity, i)
            exp = expected_slots([w[0] for w in want], [len(w[0]) for w in want], stride, seed, n)
            got = out.cpu().numpy()
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (f"stride {stride} capacity {capacity}: {bad.size} bytes differ, first at {bad[0]} "
                                   f"(slot {bad[0] // stride}, byte {bad[0] % stride}, lengths {[len(w[0]) for w in want]})")


@pytest.mark.parametrize("shape", ENC_SHAPES)
def test_encode_images_into_strides_shorter_than_the_stream(ctx, shape, opts):
    """dwtx_encode_images refuses a stream longer than the stride (DWTX_ERR_CAPACITY); what it wrote before that is the
    oracle's stream, exactly nbytes of it, and nothing is written past a stream or into a refused stream's slot."""
    H, W, Cn = shape
    pix = np.ascontiguousarray(_enc_pictures(shape))
    n = pix.shape[0]
    opts.set("part_images", 2)
    L = len(orc.encode(pix[1])[0])
    for stride in _enc_strides(L, 8):
        for capacity in (0, stride + 100):
            want = [orc.encode(p, capacity)[0] for p in pix]
            seed = 5 * stride + capacity
            before = _canary(n * stride + GUARD, seed)
            out = before.copy()
            lens = (C.c_size_t * n)()
            rc = ctx.lib.dwtx_encode_images(ctx.h, pix.ctypes.data, W, H, Cn, n, capacity, out.ctypes.data, stride,
                                            C.cast(lens, C.c_void_p), None)
            fits = [len(w) <= stride for w in want]
            assert rc == (0 if all(fits) else ERR_CAPACITY), (stride, capacity, rc)
            for i in range(n):
                slot, orig = out[i * stride:(i + 1) * stride], before[i * stride:(i + 1) * stride]
                m = len(want[i])
                if rc == 0:
                    assert lens[i] == m
                if rc == 0 or (slot != orig).any():   # after a refusal, the streams before it may have been written
                    assert fits[i], (stride, capacity, i)
                    assert slot[:m].tobytes() == want[i], (stride, capacity, i)
                    assert (slot[m:] == orig[m:]).all(), (stride, capacity, i)
            assert (out[n * stride:] == before[n * stride:]).all()


def test_encode_bound_holds_on_worst_case_8_bit_pictures(ctx):
    """nbytes <= dwtx_encode_bound(W, H, C) = 3 B/sample + 4096 on the pictures that cost an 8-bit encoder the most.
    Measured: full-range noise is the worst, ~8.75 bit/sample, 0.365 of the bound at 1080p RGB (0.36 at 256x256 gray,
    0.33 at 1000x8 gray); a period-1 0/255 checkerboard 0.12, impulses on black 0.08."""
    import torch

    import dwt_amd

    rng = np.random.default_rng(7)
    y, x = np.mgrid[:128, :128]
    check = (((x + y) & 1) * 255).astype(np.uint8)
    rb = np.zeros((128, 128, 3), np.uint8)
    rb[..., 0] = check
    rb[..., 2] = 255 - check
    imp = np.zeros((256, 256, 1), np.uint8)
    imp[rng.integers(0, 256, 500), rng.integers(0, 256, 500)] = 255
    imp3 = np.zeros((200, 200, 3), np.uint8)
    imp3[::7, ::5] = 255
    pics = [rng.integers(0, 256, (256, 256, 1), dtype=np.uint8), rng.integers(0, 256, (120, 200, 3), dtype=np.uint8),
            rng.integers(0, 256, (8, 1000, 1), dtype=np.uint8), rng.integers(0, 256, (8, 8, 3), dtype=np.uint8),
            check[..., None], np.repeat(check[..., None], 3, axis=2), rb, imp, imp3,
            rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)]
    worst = 0.0
    for p in pics:
        H, W, Cn = p.shape
        bound = ctx.lib.dwtx_encode_bound(W, H, Cn)
        dpix = torch.from_numpy(np.ascontiguousarray(p[None])).to(ctx.device)
        out = torch.empty(bound + GUARD, dtype=torch.uint8, device=ctx.device)
        info = torch.zeros((1, C.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=ctx.device)
        assert ctx.lib.dwtx_encode_device(ctx.h, dpix.data_ptr(), W, H, Cn, 1, 0, out.data_ptr(), bound, info.data_ptr()) == 0
        st = dwt_amd.StreamInfo.from_buffer_copy(info.cpu().numpy()[0].tobytes())
        assert st.error == 0 and st.nbytes <= bound, (p.shape, st.nbytes, bound)
        if p.size <= 256 * 256:
            assert out[:st.nbytes].cpu().numpy().tobytes() == orc.encode(p)[0]
        worst = max(worst, st.nbytes / bound)
    assert worst < 0.5


# ---- 3. decoder output into padded or misaligned pixel buffers ---------------------------------------------------

PIX_SHAPES = {"gray_square": (128, 128, 1), "rgb_w4": (72, 100, 3)}


@pytest.mark.parametrize("name", list(PIX_SHAPES))
def test_pictures_into_padded_and_misaligned_pixel_buffers(ctx, name):
    """pix_stride = W*H*C + {0, 1, 4, 16, 4096} and pictures 1 to 3 bytes off alignment (the unfused inverse), for a
    whole batch, a uniformly truncated one and one of mixed truncation: the pictures are the oracle's and the padding
    between them and the guard behind them keep their bytes."""
    H, W, Cn = PIX_SHAPES[name]
    fulls = [d for d, _ in streams_of(PIX_SHAPES[name])]
    orcl = Oracle(W, H, Cn)
    stride = _r8(max(len(f) for f in fulls))
    size = W * H * Cn
    batches = {
        "whole": (fulls, [len(f) for f in fulls]),
        "uniform": ([fulls[0]] * 4, [len(fulls[0]) // 3] * 4),
        "mixed": (fulls, [len(fulls[0]), len(fulls[1]) // 2, len(fulls[2]) // 9, 200]),
    }
    for what, (fs, cuts) in batches.items():
        big = layout(fs, cuts, "random", stride, seed=len(what))
        for pad, off in ((0, 0), (1, 0), (4, 0), (16, 0), (4096, 0), (0, 1), (4, 2), (16, 3)):
            infos, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn, pix_stride=size + pad, pix_off=off)
            check_pixels(orcl, fs, cuts, infos, after, before, size + pad, pix_off=off)
            sizes, hafter, hbefore = decode_images(ctx, big, stride, cuts, W, H, Cn, pix_stride=size + pad, pix_off=off)
            check_pixels(orcl, fs, cuts, None, hafter, hbefore, size + pad, pix_off=off, sizes=sizes)


@pytest.mark.parametrize("name", list(PIX_SHAPES))
def test_a_pixel_stride_below_the_picture_is_refused(ctx, name):
    H, W, Cn = PIX_SHAPES[name]
    fulls = [d for d, _ in streams_of(PIX_SHAPES[name])]
    stride = _r8(max(len(f) for f in fulls))
    cuts = [len(f) for f in fulls]
    big = layout(fulls, cuts, "random", stride)
    for ps in (W * H * Cn - 1, W * H * Cn - 4, W * H * Cn // 2):
        _, after, before = decode_device(ctx, big, stride, cuts, W, H, Cn, pix_stride=ps, expect=ERR_ARG)
        assert (after == before).all()
        _, hafter, hbefore = decode_images(ctx, big, stride, cuts, W, H, Cn, pix_stride=ps, expect=ERR_ARG)
        assert (hafter == hbefore).all()


# ---- 4. dwtx_pack_streams into a short buffer ---------------------------------------------------------------------

@pytest.mark.parametrize("stride", [64, 136])
def test_pack_streams_into_a_short_buffer(ctx, stride):
    """Nothing past out_bytes changes, the bytes before it are the packed streams', and offsets[n] is the size the
    message needs, so that a caller can tell that it was cut."""
    import torch

    rng = np.random.default_rng(stride)
    n = 7
    rows = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    lens = [0, 5, stride, 17, stride + 40, 8, 29]
    n8 = [_r8(min(v, stride)) for v in lens]
    want = np.concatenate([rows[i, :n8[i]] for i in range(n)])
    total = int(want.size)
    offs = np.concatenate([[0], np.cumsum(n8)])
    dev = torch.from_numpy(rows).to(ctx.device)
    dl = torch.tensor(lens, dtype=torch.int64, device=ctx.device)
    for out_bytes in sorted({total, total - 1, total - 8, total - 13, total // 2, 13, 8, 1}):
        before = _canary(out_bytes + GUARD, out_bytes)
        out = torch.from_numpy(before).to(ctx.device)
        offsets = torch.full((n + 1,), -1, dtype=torch.int64, device=ctx.device)
        rc = ctx.lib.dwtx_pack_streams(ctx.h, out.data_ptr(), out_bytes, offsets.data_ptr(), dev.data_ptr(), stride,
                                       dl.data_ptr(), n)
        assert rc == 0
        got = out.cpu().numpy()
        assert (got[:out_bytes] == want[:out_bytes]).all(), out_bytes
        assert (got[out_bytes:] == before[out_bytes:]).all(), out_bytes
        assert offsets.cpu().tolist() == offs.tolist()
