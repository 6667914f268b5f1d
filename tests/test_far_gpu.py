"""GPU: addresses more than 2^31 samples, or 2^32 bytes, from the pointer a call is given.

1. Far windows (dwtx_encode_view / dwtx_decode_view and their _step versions): small pictures in a frame of several GiB,
   the layouts of tests/far.py.  The frame is filled with one byte value on the device and never leaves it: the windows
   are cropped there, and after a decode the rectangles the oracle says were written are given the fill value back and
   the whole frame must hold nothing else — a store through a truncated product lands on frame (tests/test_far_cpu.py
   proves that it cannot land anywhere else), and that is where this finds it.
2. Far planes: one call whose planes together pass 2^31 samples.  A batch repeats five distinct pictures (image i is
   picture i % 5; the images on either side of 2^31 samples and the last one are different pictures): the first five
   results are compared with the oracle on the host, and on the device result i must equal result i % 5.

The yardstick is the oracle, exact, as in tests/test_views_gpu.py, whose helpers this file uses.  Every test makes a context
of its own and closes it (scratch only grows: the session's context would keep tens of GiB), and skips when
torch.cuda.mem_get_info() shows less free HBM than NEED_GIB says: the peak measured on an MI355X — free memory before the
test minus the lowest seen during it, the context's scratch included — plus a quarter.  A run prints its own peak."""
import contextlib
import ctypes

import numpy as np
import pytest

import deep
import far
import orc
import test_views_gpu as V

pytestmark = pytest.mark.gpu

FILL = 0xA5
M16 = V.M16
K = 5   # distinct pictures of a batch

# test or case -> (GiB measured, GiB below which the test skips = measured * 1.25, rounded up)
NEED_GIB = {
    "stack-rgb8-wide": (6.60, 9), "stack-gray8-general": (6.26, 8), "stack5-rgb8-wide": (6.29, 8), "grid-gray8-wide": (8.26, 11),
    "grid-rgb16-general": (16.27, 21), "planar-cs-rgb8-wide": (6.26, 8), "planar-cs-rgb16-general": (12.26, 16),
    "planar-img-rgb16-wide": (12.26, 16), "planar-img-rgb8-general": (6.26, 8), "rgbx8-rgb-wide": (6.26, 8), "rgbx8-alpha-general": (6.26, 8),
    "far-row-rgb8-wide": (6.45, 9), "far-row-gray8-general": (6.45, 9), "stack-gray16-bytes-wide": (8.26, 11),
    "stack-rgb16-both-general": (12.26, 16), "refusals": (0.31, 1),
    "transform": (19.52, 25), "pixels8": (10.48, 14), "pixels16": (12.56, 16), "linearize": (16.64, 21),
    "codec-small": (65.75, 83), "codec-small16": (62.77, 79), "codec-large": (58.62, 74),
}


# ---- a context, a memory gate and a peak meter per test ---------------------------------------------------------------

class Peak:
    def __init__(self, what):
        import torch

        self.torch, self.what = torch, what
        self.start = self.low = torch.cuda.mem_get_info()[0]

    def look(self):
        self.torch.cuda.synchronize()
        self.low = min(self.low, self.torch.cuda.mem_get_info()[0])

    def report(self):
        print(f"PEAK {self.what}: {(self.start - self.low) / 2**30:.2f} GiB of {self.start / 2**30:.1f} GiB free")


@contextlib.contextmanager
def far_context(what, peak=None, **options):
    """-> (context of its own, Peak); skips when too little HBM is free; closes the context and gives torch's cache back.
    peak: the meter of an earlier context of the same test (the codec tests: one to encode, one to decode)."""
    import torch

    import dwt_amd

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.empty_cache()
    if peak is None:
        need, free = NEED_GIB[what][1], torch.cuda.mem_get_info()[0]
        if free < need * 2**30:
            pytest.skip(f"needs about {need} GiB of free HBM ({free / 2**30:.1f} GiB free)")
        peak = Peak(what)
    c = dwt_amd.Context(0)
    try:
        for name, value in options.items():
            c.set_option(name, value)
        yield c, peak
        peak.look()
        peak.report()
    except dwt_amd.DwtxError as e:
        if e.rc == -4:   # DWTX_ERR_DEVICE: nothing more is started on a device that may have faulted
            pytest.exit(f"{what}: the device reported an error, the session ends here: {e}", returncode=3)
        raise
    finally:
        c.close()
        torch.cuda.empty_cache()


def fill_of(is16):
    """the fill byte twice, as torch's int16 holds it"""
    return (FILL * 257) - 65536 if is16 else FILL


def strays(frame, value, chunk=1 << 28):
    """-> the first few places of the flat device tensor `frame` that do not hold `value` ([] if it is nothing else)"""
    import torch

    bad = torch.zeros((), dtype=torch.bool, device=frame.device)
    for a in range(0, frame.numel(), chunk):
        bad |= (frame[a:a + chunk] != value).any()
    if not bool(bad):
        return []
    out = []
    for a in range(0, frame.numel(), chunk):
        out += (torch.nonzero(frame[a:a + chunk] != value)[:8, 0] + a).tolist()
        if len(out) >= 8:
            break
    return out


# ---- 1. far windows -------------------------------------------------------------------------------------------------------

far_cases = pytest.mark.parametrize("case", far.CASES, ids=lambda c: c.name)


def new_frame(c, case):
    import torch

    frame = torch.empty(case.L.samples, dtype=torch.int16 if case.is16 else torch.uint8, device=c.device)
    frame.fill_(fill_of(case.is16))
    return frame


def windows_of(case, frame):
    tv = case.L.t_view(frame)
    wins = [tv[i] for i in range(case.L.n)] if tv.dim() == 4 else [tv[i // tv.shape[1], i % tv.shape[1]] for i in range(case.L.n)]
    return tv, wins


def picture_of(case, i):
    return V.picture(case.W, case.H, case.Cn, case.is16, i)


def encode_far(c, case, frame, peak):
    """Pictures into the windows (on the device), one encode of the view: the oracle's bytes for the crops, and the frame
    around the windows is what it was."""
    import torch

    W, H, Cn, is16 = case.W, case.H, case.Cn, case.is16
    tv, wins = windows_of(case, frame)
    for i, w in enumerate(wins):
        p = picture_of(case, i)
        w.copy_(torch.from_numpy(p.view(np.int16) if is16 else p).to(c.device))
    out, info = c.encode_view(tv, 0, stepped=case.stepped)
    peak.look()
    infos, host = V.infos_of(info), out.cpu().numpy()
    for i, w in enumerate(wins):
        crop = V.to_host(w.contiguous(), is16)   # cropped on the device: H x W x C samples travel
        assert (crop == picture_of(case, i)).all(), f"window {i} does not hold its picture"
        want, st = V.oracle_encode(W, H, Cn, is16, i)
        assert infos[i].error == 0, i
        assert host[i, :infos[i].nbytes].tobytes() == want, f"stream {i} differs from the oracle's"
        assert (infos[i].root_bits, infos[i].total_bits) == (st.root_bits, st.total_bits), i
        w.fill_(fill_of(is16))
    bad = strays(frame, fill_of(is16))
    assert not bad, f"an encode wrote the frame at samples {bad}"


def decode_far(c, case, frame, rows, pixels_max, peak):
    """One decode into the view of a frame that holds the fill value: the oracle's picture in each window's corner, and
    once those rectangles hold the fill value again, nothing else in the whole frame."""
    import torch

    W, H, Cn, is16 = case.W, case.H, case.Cn, case.is16
    fv = fill_of(is16)
    tv, wins = windows_of(case, frame)
    stride = (max(len(r) for r in rows) + 64 + 7) // 8 * 8
    host = np.full((len(rows), stride), 0x5A, dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    streams = torch.from_numpy(host).to(c.device)
    lens = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=c.device)
    c.decode_view(streams, lens, tv, maxval=M16 if is16 else None, levels_max=deep.levels_max(W, H, pixels_max), stepped=case.stepped)
    peak.look()
    wrong = []
    for i, (w, data) in enumerate(zip(wins, rows)):
        ref = V.oracle_decode(data, W, H, Cn, is16, pixels_max)
        if ref is None:
            continue
        oh, ow = ref.shape[:2]
        got = V.to_host(w[:oh, :ow].contiguous(), is16)
        if not (got == ref).all():
            wrong.append((i, int((got != ref).sum())))
        w[:oh, :ow] = fv   # exactly the rectangle the oracle says was written
    bad = strays(frame, fv)
    assert not wrong, f"windows (index, samples that differ from the oracle's decode): {wrong}; stray samples at {bad}"
    assert not bad, f"samples outside the written rectangles changed, first at {bad} (view origin {case.L.off}, strides {case.L.strides})"


@far_cases
def test_far_windows_encode_like_the_oracle(case):
    """dwtx_encode_view[_step] on windows 2^31 samples and more from the view's origin: the oracle's bytes for the dense
    crops.  Measured peak / skip threshold per case: NEED_GIB."""
    with far_context(case.name) as (c, peak):
        frame = new_frame(c, case)
        encode_far(c, case, frame, peak)
        del frame


@far_cases
def test_far_windows_decode_and_nothing_else_is_written(case):
    """dwtx_decode_view[_step]: whole, cut, mixed and level-capped streams into far windows; the windows hold the oracle's
    decode (a cut or capped stream only in its ow x oh corner) and no other sample of the frame changes.  Measured peak /
    skip threshold per case: NEED_GIB."""
    with far_context(case.name) as (c, peak):
        frame = new_frame(c, case)
        for name, rows, pixels_max in V.decode_cases(case.W, case.H, case.Cn, case.is16, case.L.n):
            print(name)
            decode_far(c, case, frame, rows, pixels_max, peak)
        del frame


SWITCHES = [("decode_parts", 2), ("decode_parts", 4), ("lift_rows", 16), ("lift_rows", 64)]


@pytest.mark.parametrize("name,value", SWITCHES, ids=["%s=%d" % s for s in SWITCHES])
@pytest.mark.parametrize("case", [far.BY_NAME[n] for n in far.SWITCHED], ids=lambda c: c.name)
def test_far_windows_under_the_switches(case, name, value):
    """A far stack (the wide kernels) and a far grid (the general conversions) with the decoder's batch cut into 2 and 4
    parts — a part's first window is then a far one — and with 16 and 64 row pairs per wave strip."""
    with far_context(case.name, **{name: value}) as (c, peak):
        frame = new_frame(c, case)
        encode_far(c, case, frame, peak)
        for cname, rows, pixels_max in V.decode_cases(case.W, case.H, case.Cn, case.is16, case.L.n)[::2]:   # whole, mixed
            print(cname)
            decode_far(c, case, frame, rows, pixels_max, peak)
        del frame


# ---- what is 32-bit by design is refused ----------------------------------------------------------------------------------

def test_counts_beyond_a_grid_dimension_are_refused_with_a_message():
    """The planes of one call are a grid dimension of its launches (at most 65535), the decoder takes
    21845 streams: one more is DWTX_ERR_ARG with a text, from every entry point that takes a count, before anything runs.
    Measured peak / skip threshold: NEED_GIB["refusals"]."""
    import torch

    import dwt_amd

    with far_context("refusals") as (c, peak):
        dev = c.device
        P = 65536
        planes = torch.zeros((P, 8, 8), dtype=torch.int32, device=dev)
        pix = torch.zeros((P, 8, 8, 1), dtype=torch.uint8, device=dev)
        rgb = torch.zeros((21846, 8, 8, 3), dtype=torch.uint8, device=dev)
        lens = torch.full((21846,), 64, dtype=torch.int64, device=dev)
        streams = torch.zeros((21846, 64), dtype=torch.uint8, device=dev)
        calls = {
            "transformation_fwd": lambda: c.transformation_fwd(planes),
            "transformation_inv": lambda: c.transformation_inv(planes),
            "linearization": lambda: c.linearization(planes),
            "reconstruction": lambda: c.reconstruction(planes.view(P, 64), 8, 8, 1),
            "encode_device gray": lambda: c.encode_device(pix),
            "encode_device rgb": lambda: c.encode_device(rgb),
            "encode_view": lambda: c.encode_view(pix),
            "decode_device": lambda: c.decode_device(streams, lens, 8, 8, 1),
            "decode_view": lambda: c.decode_view(streams, lens, pix[:21846]),
            "pack_streams": lambda: c.pack_streams(torch.zeros((P, 8), dtype=torch.uint8, device=dev), torch.zeros(P, dtype=torch.int64, device=dev),
                                                   torch.zeros(P * 8, dtype=torch.uint8, device=dev)),
        }
        for what, call in calls.items():
            with pytest.raises(dwt_amd.DwtxError, match=r"in one call: at most (65535|21845)") as e:
                call()
            assert e.value.rc == V.ERR_ARG, what
        # the largest counts are taken
        c.transformation_fwd(planes[:65535])
        c.sync()
        # a pixel step that does not fit the kernels' int
        v = dwt_amd.View(pix.data_ptr(), 1, 1, 255, 0, 1 << 40, 1 << 41, 0, 0)
        info = torch.zeros((1, 128), dtype=torch.uint8, device=dev)
        assert c.lib.dwtx_encode_view_step(c.h, v, 1 << 31, 8, 8, 1, 0, streams.data_ptr(), 64, info.data_ptr()) == V.ERR_ARG
        assert b"pixel_step" in c.lib.dwtx_last_error()


# ---- 2. far planes --------------------------------------------------------------------------------------------------------

SMALL, LARGE = (260, 256), (4096, 4096)   # W, H: the LDS tail, the one-level and the two-level kernels all run | few large planes
T31 = 1 << 31
_refs = {}


def cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def batch_of(base, n):
    """device tensor [K, ...] -> [n, ...], image i = picture i % K"""
    import torch

    return base[torch.arange(n, device=base.device) % K]


def check_far_batch(n, samples_per_image):
    """the batch passes 2^31 samples, and the images on either side of that line and the last one are different pictures"""
    total = n * samples_per_image
    line = T31 // samples_per_image   # the image sample 2^31 lies in (or begins)
    assert total > T31 and 0 < line < n and len({(line - 1) % K, line % K}) == 2 and (n - 1) % K != (line - 1) % K, (n, samples_per_image)


def off_period(t, but=()):
    """t: device tensor [n, ...] -> the sorted indices i, other than those in `but`, at which t[i] != t[i % K]"""
    import torch

    flat = t.reshape(t.shape[0], -1)
    step = max(1, (1 << 28) // flat.shape[1])
    bad = []
    for r in range(K):
        rows = flat[r::K]
        for a in range(0, rows.shape[0], step):
            ne = (rows[a:a + step] != flat[r]).any(dim=1)
            bad += ((torch.nonzero(ne)[:, 0] + a) * K + r).tolist()
    return sorted(set(bad) - set(but))


def first_equal(t, want, what):
    """the first K entries of the device tensor against the oracle's (numpy), on the host"""
    got = t[:len(want)].cpu().numpy()
    for i, w in enumerate(want):
        assert (got[i].reshape(w.shape) == w).all(), f"{what}: entry {i} differs from the oracle's"


regimes = pytest.mark.parametrize("regime", ["small", "large"])


def planes_of(regime):
    """-> (W, H, planes in one call)"""
    return SMALL + (33000,) if regime == "small" else LARGE + (130,)


@regimes
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "one-level"])
def test_far_planes_transform_both_ways(regime, fused):
    """dwtx_transformation_fwd / _inv on int32 planes that together pass 2^31 samples (33000 of 260x256, 130 of 4096x4096),
    two levels per pass and one (no_fused_levels): `plane * src_ps`, `plane * det_ps` and the scratch planes' strides at the
    far end.  Measured peak / skip threshold: NEED_GIB["transform"]."""
    import torch

    W, H, P = planes_of(regime)
    check_far_batch(P, W * H)
    base = cached(("planes", regime), lambda: np.random.default_rng(W).integers(-5000, 5000, size=(K, H, W), dtype=np.int32))
    want = cached(("pyr", regime), lambda: [orc.forward(b[:, :, None])[:, :, 0] for b in base])
    with far_context("transform", no_fused_levels=0 if fused else 1) as (c, peak):
        planes = batch_of(torch.from_numpy(base).to(c.device), P)
        pyr = c.transformation_fwd(planes)
        peak.look()
        assert off_period(pyr) == []
        first_equal(pyr, want, "forward")
        back = c.transformation_inv(pyr, out=planes.zero_())
        peak.look()
        assert off_period(back) == []
        first_equal(back, list(base), "inverse")
        del planes, pyr, back


def rgb_pictures(regime, is16):
    """K RGB pictures; deep ones have maxval 4095 (the large ones are the bytes' times 16 plus a little: cheap to make)"""
    W, H = SMALL if regime == "small" else LARGE

    def one(i):
        if not is16:
            return orc.synth(W, H, 3, 40 + i, 0)
        return deep.smooth_noise(W, H, 3, M16, seed=40 + i) if regime == "small" else orc.synth(W, H, 3, 40 + i, 0).astype(np.uint16) * 16 + 3 * i

    return cached(("rgb", regime, is16), lambda: [one(i) for i in range(K)])


def device_pictures(c, pics, is16):
    import torch

    a = np.stack(pics)
    return torch.from_numpy(a.view(np.int16) if is16 else a).to(c.device)


@regimes
@pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
def test_far_pixels_to_planes_and_back(regime, is16):
    """dwtx_planes_from_pixels[16] / dwtx_pixels[16]_from_planes on RGB batches past 2^31 samples (11000 of 260x256, 43 of
    4096x4096): the conversions' `win * C * npix` and `win_off`.  Measured peak / skip threshold: NEED_GIB["pixels8" / "pixels16"]."""
    import torch

    W, H = SMALL if regime == "small" else LARGE
    n = 11000 if regime == "small" else 43
    check_far_batch(n, W * H * 3)
    pics = rgb_pictures(regime, is16)
    want = cached(("ycocg", regime, is16), lambda: [np.ascontiguousarray(np.moveaxis(deep.rgb2ycocg(p), 2, 0)) for p in pics])
    with far_context("pixels16" if is16 else "pixels8") as (c, peak):
        pix = batch_of(device_pictures(c, pics, is16), n)
        planes = (c.planes_from_pixels16 if is16 else c.planes_from_pixels)(pix)
        peak.look()
        assert off_period(planes.view(n, 3, H, W)) == []
        first_equal(planes.view(n, 3, H, W), want, "planes")
        del pix
        back = c.pixels16_from_planes(planes, 3, M16).view(torch.int16) if is16 else c.pixels_from_planes(planes, 3)
        peak.look()
        assert off_period(back) == []
        first_equal(back, [p.view(np.int16) if is16 else p for p in pics], "pixels")
        del planes, back


@regimes
def test_far_linearization_and_reconstruction(regime):
    """dwtx_linearization / dwtx_reconstruction past 2^31 samples: 11000 RGB pyramids of 260x256 with a `missing` table of
    their own each (decode.c:51-58's bias), 130 gray ones of 4096x4096 without.  Measured peak / skip threshold:
    NEED_GIB["linearize"]."""
    import torch

    W, H = SMALL if regime == "small" else LARGE
    Cn, n = (3, 11000) if regime == "small" else (1, 130)
    check_far_batch(n, W * H * Cn)
    g = orc.geometry(W, H)

    def make():
        rng = np.random.default_rng(H)
        pyr = rng.integers(-40, 40, size=(K, Cn, H, W), dtype=np.int32)
        pyr[rng.random(pyr.shape) < 0.5] = 0
        lin = [orc.linearize(np.ascontiguousarray(np.moveaxis(p, 0, 2))) for p in pyr]
        missing = np.zeros((K, 3, 16), dtype=np.int32)
        if regime == "small":
            missing[:, :Cn, :g.levels] = rng.integers(0, 7, size=(K, Cn, g.levels))
        rec = [np.ascontiguousarray(np.moveaxis(orc.reconstruct(l, W, H, g.levels, m.reshape(-1)), 2, 0)) for l, m in zip(lin, missing)]
        return pyr, lin, missing, rec

    pyr, lin_want, missing, rec_want = cached(("lin", regime), make)
    with far_context("linearize") as (c, peak):
        batch = batch_of(torch.from_numpy(pyr).to(c.device), n).view(n * Cn, H, W)
        lin = c.linearization(batch)
        peak.look()
        assert off_period(lin.view(n, -1)) == []
        first_equal(lin.view(n, Cn, W * H), lin_want, "linearised")
        del batch
        table = batch_of(torch.from_numpy(missing).to(c.device), n).contiguous().view(-1) if regime == "small" else None
        rec = c.reconstruction(lin, W, H, Cn, missing=table)
        peak.look()
        assert off_period(rec.view(n, -1)) == []
        first_equal(rec.view(n, Cn, H, W), rec_want, "reconstructed")
        del lin, rec


# ---- the codec ------------------------------------------------------------------------------------------------------------

def coded(pics, is16):
    """-> [(stream, stats)] of the K pictures, from the oracle"""
    return [deep.deep_encode(p) if is16 else orc.encode(p) for p in pics]


def oracle_back(blob, W, H, Cn, is16):
    return cached(("back", is16, blob), lambda: deep.deep_decode(blob, W, H, Cn, M16) if is16 else orc.decode(blob))


def codec_round_trip(what, pics, streams_want, n, is16, index, tag, **options):
    """encode_device[16] of the batch, then decode_device[16] of its streams with a few near the far end replaced by cut
    and damaged copies.  pics: the K pictures [H, W, C]; streams_want: the oracle's streams of them.  The encode and the
    decode have a context each, one after the other: the first one's scratch is given back before the second asks for its
    own, which halves what the test needs."""
    import torch

    from refsweep import corrupted_blobs
    from test_encode_index_gpu import _assert_equal, _decoder_made

    import dwt_amd

    H, W, Cn = pics[0].shape
    check_far_batch(n, W * H * Cn)
    with far_context(what, **options) as (c, peak):
        pix = batch_of(device_pictures(c, pics, is16), n)
        bound = (c.lib.dwtx_encode_bound16 if is16 else c.lib.dwtx_encode_bound)(W, H, Cn)
        assert n * bound > 1 << 32, "the encoder's stream buffer passes 2^32 bytes"
        out = torch.zeros((n, bound), dtype=torch.uint8, device=c.device)   # (zeros: a slot's bytes past its stream's padding are left as they were)
        info = torch.zeros((n, ctypes.sizeof(dwt_amd.StreamInfo)), dtype=torch.uint8, device=c.device)
        ix = c.set_encode_index(n, device=True).zero_() if index else None
        try:
            (c.encode_device16 if is16 else c.encode_device)(pix, 0, out=out, info=info)
            c.sync()
        finally:
            c.set_encode_index()
        peak.look()
        del pix
        lens = c.stream_lengths(info).clone()
        assert off_period(info) == [] and off_period(out) == [], "stream i is not stream i % 5"
        host_lens = lens[:K].cpu().numpy()
        for i, (want, st) in enumerate(streams_want):
            assert int(host_lens[i]) == len(want) and out[i, :len(want)].cpu().numpy().tobytes() == want, f"stream {i} differs from the oracle's"
        if index:   # entry i belongs to image i at the far end too
            assert off_period(ix) == []
            enc = [dwt_amd.index_from_row(r) for r in ix[:K].cpu()]
            made, _, _ = _decoder_made(c, [s for s, _ in streams_want], W, H, Cn)
            _assert_equal(enc, made, tag)
        del ix
        # the decoder's tables are laid out per stream stride, and the encoder's is a worst-case bound: a stride that fits the
        # streams and still puts the last of them more than 2^32 bytes from the first
        stride = (max(int(lens.max()) + 64, (1 << 32) // (n - 1) + 8) + 7) // 8 * 8
        assert stride <= bound and (n - 1) * stride > 1 << 32
        streams = out[:, :stride].contiguous()
        del out, info
    # decode: cut copies near the far end (the non-uniform parts: one finish per image at a far `first`), one damaged copy
    whole = [s for s, _ in streams_want]
    changed = {n - 2: V.cut(whole[(n - 2) % K], streams_want[(n - 2) % K][1]), n - 7: V.cut(whole[(n - 7) % K], streams_want[(n - 7) % K][1]),
               n - 4: corrupted_blobs(whole[(n - 4) % K], 2, 11)[1]}
    with far_context(what, peak=peak, **options) as (c, peak):
        for i, blob in changed.items():
            streams[i, :len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(c.device)
            lens[i] = len(blob)
        back = torch.full((n, W * H * Cn), fill_of(is16), dtype=torch.int16 if is16 else torch.uint8, device=c.device)
        if is16:
            _, infos = c.decode_device16(streams, lens, W, H, Cn, M16, out=back)
        else:
            _, infos = c.decode_device(streams, lens, W, H, Cn, out=back)
        peak.look()
        assert all(I.status == 0 and not I.truncated for i, I in enumerate(infos) if i not in changed)
        assert off_period(back, but=changed) == [], "picture i is not picture i % 5"
        first_equal(back, [(p.view(np.int16) if is16 else p).reshape(-1) for p in pics], "decoded")
        for i, blob in changed.items():
            ref = oracle_back(blob, W, H, Cn, is16)
            got = V.to_host(back[i], is16)
            k = 0 if ref is None else ref.size
            assert (ref is None) == (infos[i].status != 0), i
            assert k == 0 or (got[:k] == ref.reshape(-1)).all(), f"image {i} (a {'cut' if i != n - 4 else 'damaged'} stream) differs from the oracle's decode"
            assert (got[k:] == (FILL * 257 if is16 else FILL)).all(), f"image {i}: its slot was written past the picture"
        del streams, back


MODES = {"one-part": dict(one_stream=1), "parts": {}, "no-fine16": dict(no_fine16=1), "no-square-tiles": dict(no_square_tiles=1)}


@pytest.mark.parametrize("mode", list(MODES))
def test_far_codec_many_small_pictures(mode):
    """dwtx_encode_device then dwtx_decode_device on 11000 RGB pictures of 260x256 (33000 planes, 2.2e9 samples, 6.6 GB of
    encoder stream slots, 4.3 GB of them for the decoder): as one part (one_stream keeps the encoder's and the decoder's batch whole), in the automatic four parts
    (the last part's `first` is a far one on both sides), and once each without the 16-bit ring planes and without tiles read
    in place.  The first two collect the encoder's sidecar index as well.  Measured peak / skip threshold: NEED_GIB["codec-small"]."""
    pics = rgb_pictures("small", False)
    want = cached(("coded", "small", False), lambda: coded(pics, False))
    codec_round_trip("codec-small", pics, want, 11000, False, mode in ("one-part", "parts"), mode, **MODES[mode])


def test_far_codec_many_small_deep_pictures():
    """dwtx_encode_device16 / dwtx_decode_device16, maxval 4095, on the same count of 16-bit pictures: byte offsets are
    twice the sample offsets.  Measured peak / skip threshold: NEED_GIB["codec-small16"]."""
    pics = rgb_pictures("small", True)
    want = cached(("coded", "small", True), lambda: coded(pics, True))
    codec_round_trip("codec-small16", pics, want, 11000, True, False, "deep")


@pytest.mark.parametrize("mode", ["one-part", "parts"])
def test_far_codec_few_large_pictures(mode):
    """130 gray pictures of 4096x4096 (2^31 samples and 2 pictures): the encoder's four parts start at images 32, 65 and 97,
    the decoder's too; one_stream keeps both whole.  Measured peak / skip threshold: NEED_GIB["codec-large"]."""
    W, H = LARGE
    pics = cached(("gray", "large"), lambda: [orc.synth(W, H, 1, 60 + i, 0) for i in range(K)])
    want = cached(("coded", "large"), lambda: coded(pics, False))
    codec_round_trip("codec-large", pics, want, 130, False, False, mode, **MODES[mode])
