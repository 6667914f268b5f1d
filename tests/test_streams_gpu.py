"""GPU: the stream, context and thread contracts of include/dwtx.h.

"All functions are asynchronous on the context's stream", "one context per host thread", dwtx_ctx_create_on_stream on
the caller's stream, dwtx_stream() to chain other streams: the codec runs most of its work on side streams (encoder
parts from 128 images on, decoder parts from 4, a copy stream for the host-buffer pipelines) that fork from and join
the caller's stream through events the context reuses from call to call.  The rest of the suite shares one context on
the default stream and reads every result back with .cpu(); here the contexts live on streams of their own and nothing
synchronises between the calls.

The method, for whoever adds a side stream:
  - a *delay* (a benign busy kernel, calibrated once per module) is queued on the caller's stream in front of the
    producer of a call's input.  Work that the library forks without waiting for the caller's stream then runs before
    the producer;
  - the input buffer holds a *decoy* until the producer runs — another valid picture (other valid streams with valid
    lengths for the decoder) — and is overwritten with a second decoy right after the call, on the same stream, while
    clones of the outputs are queued behind that.  A lost fork or join shows as the decoy's bytes, or as unfinished
    output, never as a fault;
  - a test that relies on the delay measures it (stream events) and the GPU time of a warm run of the call, prints
    both, and FAILS as inconclusive unless the delay is at least 5 times the call.

Yardsticks: tests/orc.py and tests/deep.py; every comparison is exact."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu

ERR_ARG = -3
GUARD = 4096          # sentinel samples behind the last picture slot
PAD = 40              # sentinel samples between picture slots
FRONT = 24            # sentinel samples before the first
HEAD = 32             # bytes of dwtx_index before seg[]
M16 = 4095            # maxval of the deep pictures
POOL = 7              # distinct pictures per geometry: picture i of a batch is pool[i % 7]
WIDE, ODD = (96, 80, 3), (77, 53, 3)   # W, H, C: the fused wide path; widened planes


@pytest.fixture(autouse=True)
def _need_gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _r8(v):
    return (v + 7) // 8 * 8


# ---- pictures and what the oracle makes of them (computed once, shared, never changed) ------------------------------

@functools.lru_cache(maxsize=None)
def _pool(depth, W, H, Cn):
    if depth == 8:
        pics = [orc.synth(W, H, Cn, 31 + k, k & 1) for k in range(POOL)]
    else:
        pics = [deep.smooth_noise(W, H, Cn, M16, 1 + k) if k % 3 else deep.blocks(W, H, Cn, M16, 1 + k) for k in range(POOL)]
    for p in pics:
        p.setflags(write=False)
    return tuple(pics)


@functools.lru_cache(maxsize=None)
def _streams(depth, W, H, Cn):
    """-> 7 x (.dwt bytes, orc.Stats), all different."""
    enc = tuple((orc.encode(p) if depth == 8 else deep.deep_encode(p)) for p in _pool(depth, W, H, Cn))
    assert len({d for d, _ in enc}) == POOL, "the pool's pictures must encode to different streams"
    return enc


@functools.lru_cache(maxsize=None)
def _decoded(depth, W, H, Cn, k, cut):
    """The oracle's picture of the first `cut` bytes of pool stream k (None: unreadable)."""
    data = _streams(depth, W, H, Cn)[k][0][:cut]
    ref = orc.decode(data) if depth == 8 else deep.deep_decode(data, W, H, Cn, M16)
    if ref is not None:
        ref.setflags(write=False)
    return ref


def _np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _device_pixels(dev, depth, W, H, Cn, n, shift):
    """[n, H, W, C] on the device, picture i = pool[(i + shift) % 7] (deep ones as int16: the same two bytes)."""
    import torch

    pool = _pool(depth, W, H, Cn)
    arr = np.stack([pool[(i + shift) % POOL] for i in range(n)])
    return torch.from_numpy(arr if depth == 8 else arr.view(np.int16)).to(dev)


def _row_of(depth, W, H, Cn, i, shift):
    """(pool index, byte count) of stream row i: whole streams and two prefixes, 2/7 and 5/7 into what follows the root
    image, in turn."""
    k = (i + shift) % POOL
    data, st = _streams(depth, W, H, Cn)[k]
    L = len(data)
    if i % 3 == 0:
        return k, L
    hdr = (st.meta_bits + st.root_bits + 7) // 8
    return k, hdr + (L - hdr) * (2 if (i + shift) % 2 else 5) // 7


def _first_diff(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.size != want.size:
        return f"sizes {got.size} != {want.size}"
    bad = np.nonzero(got != want)[0]
    return "equal" if bad.size == 0 else f"{bad.size} differ, first at {int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}"


def _differ(a, b):
    """Two decoded pictures (None: unreadable) are not the same."""
    if a is None or b is None:
        return (a is None) != (b is None)
    return a.shape != b.shape or bool((a != b).any())


def _infos(info_np):
    import dwt_amd

    return [dwt_amd.StreamInfo.from_buffer_copy(info_np[i].tobytes()) for i in range(info_np.shape[0])]


def _check_streams(out_np, info_np, depth, W, H, Cn, shift, what=""):
    """Streams and StreamInfo records of a batch whose picture i is pool[(i + shift) % 7] against the oracle."""
    enc = _streams(depth, W, H, Cn)
    for i, I in enumerate(_infos(info_np)):
        want, st = enc[(i + shift) % POOL]
        where = f"{what} image {i} of {info_np.shape[0]}"
        assert I.error == 0, where
        assert I.nbytes == len(want), f"{where}: nbytes {I.nbytes}, the oracle's stream has {len(want)}"
        assert I.total_bits == st.total_bits, where
        assert list(I.planes)[:Cn] == list(st.planes)[:Cn], where
        got = out_np[i, :len(want)]
        assert got.tobytes() == want, f"{where}: {_first_diff(got, np.frombuffer(want, dtype=np.uint8))}"


# ---- contexts -------------------------------------------------------------------------------------------------------

def _context_on(S):
    import dwt_amd

    return dwt_amd.Context(0, stream=S.cuda_stream)


def _context_with_own_stream():
    """A Context around dwtx_ctx_create (a stream of the library's own making), as the CLIs use it."""
    import torch

    import dwt_amd
    from dwt_amd import _lib

    c = object.__new__(dwt_amd.Context)
    c.torch, c.lib, c.device = torch, _lib.load(), torch.device("cuda", 0)
    h = C.c_void_p()
    rc = c.lib.dwtx_ctx_create(0, C.byref(h))
    assert rc == 0, c.lib.dwtx_last_error()
    c.h = h
    return c


# ---- the delay ------------------------------------------------------------------------------------------------------

class _Delay:
    """A benign busy kernel on the current stream: torch.cuda._sleep, or a chain of matmuls where that does not scale
    with its argument.  Calibrated once with stream events."""

    def __init__(self):
        import torch

        self.torch = torch
        self.per_ms = None        # cycles (or matmuls) per millisecond
        self.x = None
        S = torch.cuda.Stream()
        with torch.cuda.stream(S):
            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                S.synchronize()
                return e0.elapsed_time(e1)

            N = 4_000_000
            timed(lambda: torch.cuda._sleep(N))
            t1, t2 = timed(lambda: torch.cuda._sleep(N)), timed(lambda: torch.cuda._sleep(3 * N))
            if t1 > 0.05 and 2.0 < t2 / t1 < 4.0:
                self.per_ms = 2 * N / (t2 - t1)
                print(f"delay: torch.cuda._sleep, {self.per_ms:.0f} cycles per ms ({N} cycles {t1:.2f} ms, {3 * N} cycles {t2:.2f} ms)")
                return
            self.x = torch.randn(4096, 4096, device="cuda")

            def chain(k):
                y = self.x
                for _ in range(k):
                    y = y @ self.x
                    y = y / 4096.0

            timed(lambda: chain(4))
            t = timed(lambda: chain(16))
            self.per_ms = 16 / t
            print(f"delay: _sleep does not scale ({t1:.2f}, {t2:.2f} ms); matmul chain, {self.per_ms:.2f} links per ms")

    def queue(self, ms):
        """~ms milliseconds of busy kernel on torch's current stream."""
        if self.x is None:
            self.torch.cuda._sleep(int(ms * self.per_ms))
            return
        y = self.x
        for _ in range(max(1, int(ms * self.per_ms + 0.5))):
            y = y @ self.x
            y = y / 4096.0


@pytest.fixture(scope="module")
def delay():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _Delay()


def _delay_for(call_ms):
    """The delay to ask for: about 40 ms, and 8 times the call's own GPU time if that is more (the test then checks the
    ratio of what was measured)."""
    return min(max(40.0, 8.0 * call_ms), 1500.0)


def _conclusive(what, delay_ms, call_ms):
    print(f"{what}: delay {delay_ms:.2f} ms, the call's own GPU time (warm) {call_ms:.3f} ms, ratio {delay_ms / max(call_ms, 1e-6):.1f}")
    if delay_ms < 5.0 * call_ms:
        pytest.fail(f"{what}: inconclusive — the delay ({delay_ms:.2f} ms) is not 5 times the call's own time ({call_ms:.3f} ms)")


def _events(n):
    import torch

    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


# ---- calls as steps: stage once, queue on the current stream, check after the synchronisation ------------------------
# queue(c) is called inside `with torch.cuda.stream(S)` for the context's stream S.  It fills the call's input on S
# (the buffer holds a decoy until then), makes the call, overwrites the input with a second decoy, and returns the
# tensors to keep — outputs first — none of which is read before the caller synchronises.

class _Enc:
    """encode_device / encode_device16 of n pictures of one geometry."""

    def __init__(self, dev, depth, geom, n, shift=0):
        W, H, Cn = geom
        self.depth, self.geom, self.n, self.shift = depth, geom, n, shift
        self.real = _device_pixels(dev, depth, W, H, Cn, n, shift)
        self.decoy = _device_pixels(dev, depth, W, H, Cn, n, shift + 3)
        self.decoy2 = _device_pixels(dev, depth, W, H, Cn, n, shift + 5)
        enc = _streams(depth, W, H, Cn)
        for k in range(POOL):   # a decoy picture encodes to something else than the picture it stands in for
            assert enc[k][0] != enc[(k + 3) % POOL][0] and enc[k][0] != enc[(k + 5) % POOL][0]
        self.what = f"encode{'' if depth == 8 else '16'} {W}x{H}x{Cn} n={n}"

    def call(self, c, pix, out=None, info=None):
        return (c.encode_device if self.depth == 8 else c.encode_device16)(pix, out=out, info=info)

    def queue(self, c):
        pix = self.decoy.clone()
        pix.copy_(self.real)
        out, info = self.call(c, pix)
        pix.copy_(self.decoy2)
        return out, info, pix

    def check(self, kept):
        W, H, Cn = self.geom
        _check_streams(kept[0], kept[1], self.depth, W, H, Cn, self.shift, self.what)

    def results(self, kept):
        """What the call defines of its outputs, to compare two runs with: the stream lengths and the streams (a slot's
        bytes past its stream are the caller's)."""
        lens = np.array([I.nbytes for I in _infos(kept[1])])
        return [lens] + [kept[0][i, :L] for i, L in enumerate(lens)]


class _Dec:
    """dwtx_decode_device / dwtx_decode_device16 of n stream rows — whole streams and prefixes — into picture slots with
    sentinels before, between and behind them."""

    def __init__(self, dev, depth, geom, n, shift=0, whole=False):
        import torch

        W, H, Cn = geom
        self.depth, self.geom, self.n = depth, geom, n
        enc = _streams(depth, W, H, Cn)
        self.stride = _r8(max(len(d) for d, _ in enc) + 64)
        self.pix_stride = W * H * Cn + PAD

        def rows(sh):
            host = np.zeros((n, self.stride), dtype=np.uint8)
            lens, which = [], []
            for i in range(n):
                k, L = ((i + sh) % POOL, len(enc[(i + sh) % POOL][0])) if whole else _row_of(depth, W, H, Cn, i, sh)
                host[i, :L] = np.frombuffer(enc[k][0][:L], dtype=np.uint8)
                lens.append(L)
                which.append((k, L))
            return torch.from_numpy(host).to(dev), torch.tensor(lens, dtype=torch.int64, device=dev), which

        self.rows, self.lens, self.which = rows(shift)
        self.decoy_rows, self.decoy_lens, decoy_which = rows(shift + 3)
        self.decoy2_rows, self.decoy2_lens, decoy2_which = rows(shift + 5)
        self.before = np.random.default_rng(n + W).integers(0, 256 if depth == 8 else 65536, FRONT + n * self.pix_stride + GUARD,
                                                              dtype=_np_dtype(depth))
        self.want = self.before.copy()
        self.refs = []
        for i, (k, L) in enumerate(self.which):
            ref = _decoded(depth, W, H, Cn, k, L)
            self.refs.append(ref)
            for kk, LL in (decoy_which[i], decoy2_which[i]):   # a decoy row decodes to something else
                other = _decoded(depth, W, H, Cn, kk, LL)
                assert _differ(ref, other), i
            if ref is not None:
                o = FRONT + i * self.pix_stride
                self.want[o:o + ref.size] = ref.reshape(-1)
        assert any(r is not None and r.shape == (H, W, Cn) for r in self.refs)
        self.buf0 = torch.from_numpy(self.before if depth == 8 else self.before.view(np.int16)).to(dev)
        self.what = f"decode{'' if depth == 8 else '16'} {W}x{H}x{Cn} n={n}"

    def call(self, c, rows, lens, buf):
        import dwt_amd

        W, H, Cn = self.geom
        infos = (dwt_amd.DecodeInfo * self.n)()
        item = 1 if self.depth == 8 else 2
        args = (c.h, rows.data_ptr(), self.stride, lens.data_ptr(), W, H, Cn, self.n, -1, buf.data_ptr() + item * FRONT, self.pix_stride)
        if self.depth == 8:
            rc = c.lib.dwtx_decode_device(*args, C.cast(infos, C.c_void_p))
        else:
            rc = c.lib.dwtx_decode_device16(*args, M16, C.cast(infos, C.c_void_p))
        assert rc == 0, (self.what, rc, c.lib.dwtx_last_error())
        for i, ref in enumerate(self.refs):
            assert (infos[i].status == 0) == (ref is not None), (self.what, i)

    def queue(self, c):
        rows, lens, buf = self.decoy_rows.clone(), self.decoy_lens.clone(), self.buf0.clone()
        rows.copy_(self.rows)
        lens.copy_(self.lens)
        self.call(c, rows, lens, buf)
        rows.copy_(self.decoy2_rows)
        lens.copy_(self.decoy2_lens)
        return buf, rows, lens

    def check(self, kept):
        got = kept[0].view(_np_dtype(self.depth))
        assert (got == self.want).all(), f"{self.what}: pictures or the sentinels around them: {_first_diff(got, self.want)}"

    def results(self, kept):
        return [kept[0]]


class _RoundTrip16:
    """encode_device16, then decode_device16 of the streams where they lie, with the lengths taken from the info records
    on the device: what a torch pipeline does."""

    def __init__(self, dev, geom, n, shift=0):
        self.enc = _Enc(dev, 16, geom, n, shift)
        self.geom, self.n = geom, n
        self.what = "round trip of " + self.enc.what

    def queue(self, c):
        W, H, Cn = self.geom
        pix = self.enc.decoy.clone()
        pix.copy_(self.enc.real)
        out, info = c.encode_device16(pix)
        pix.copy_(self.enc.decoy2)
        back, _ = c.decode_device16(out, c.stream_lengths(info), W, H, Cn, M16)
        return out, info, back.view(c.torch.int16), pix

    def check(self, kept):
        self.enc.check(kept)
        want = self.enc.real.cpu().numpy().view(np.uint16).reshape(self.n, -1)
        got = kept[2].view(np.uint16)
        assert (got == want).all(), f"{self.what}: {_first_diff(got, want)}"

    def results(self, kept):
        return self.enc.results(kept) + [kept[2]]


class _Chain:
    """transformation_fwd -> linearization -> reconstruction -> transformation_inv on int32 planes."""

    def __init__(self, dev, geom, n):
        import torch

        W, H, Cn = geom
        self.geom, self.n = geom, n
        pool = _pool(8, W, H, Cn)

        def planes(shift):
            return np.ascontiguousarray(np.stack([pool[(i + shift) % POOL].astype(np.int32).transpose(2, 0, 1) for i in range(n)])).reshape(n * Cn, H, W)

        self.planes = planes(0)
        pyrs = [orc.forward(pool[i % POOL].astype(np.int32)) for i in range(n)]
        self.pyr = np.stack([p.transpose(2, 0, 1) for p in pyrs]).reshape(n * Cn, H, W)
        self.lin = np.concatenate([orc.linearize(p) for p in pyrs])
        assert (planes(3) != self.planes).any()
        self.real, self.decoy = torch.from_numpy(self.planes).to(dev), torch.from_numpy(planes(3)).to(dev)
        self.what = f"transform chain {W}x{H}x{Cn} n={n}"

    def queue(self, c):
        W, H, Cn = self.geom
        x = self.decoy.clone()
        x.copy_(self.real)
        pyr = c.transformation_fwd(x)
        x.copy_(self.decoy)
        lin = c.linearization(pyr)
        rec = c.reconstruction(lin, W, H, Cn)
        back = c.transformation_inv(rec)
        return pyr, lin, back, x, rec

    def check(self, kept):
        assert (kept[0] == self.pyr).all(), f"{self.what} pyramid: {_first_diff(kept[0], self.pyr)}"
        assert (kept[1] == self.lin).all(), f"{self.what} linearised: {_first_diff(kept[1], self.lin)}"
        assert (kept[2] == self.planes).all(), f"{self.what} back: {_first_diff(kept[2], self.planes)}"

    def results(self, kept):
        return list(kept[:3])


def _to_host(kept):
    return [t.cpu().numpy() for t in kept]


def _run(S, c, steps, delay=None, delay_ms=0.0):
    """Queue the delay (optional) and the steps on S with nothing between them, synchronise once.
    -> (kept tensors of every step as numpy, measured delay in ms, GPU time of the steps in ms)."""
    import torch

    t0, t1, t2 = _events(3)
    with torch.cuda.stream(S):
        t0.record()
        if delay is not None:
            delay.queue(delay_ms)
        t1.record()
        kept = [st.queue(c) for st in steps]
        t2.record()
    S.synchronize()
    return [_to_host(k) for k in kept], t0.elapsed_time(t1), t1.elapsed_time(t2)


# ---- 1. the encoder waits for the caller's earlier work and joins before the caller's later work ---------------------

ENCODE_CASES = {   # depth, geometry, n: one part below 128 pictures, four parts from there on
    "wide8_n3": (8, WIDE, 3), "wide8_n130": (8, WIDE, 130), "odd8_n130": (8, ODD, 130),
    "wide16_n130": (16, WIDE, 130), "odd16_n3": (16, ODD, 3),
}


def _encode_behind_delay(delay, step, c, S, index=False):
    """The test's sequence on S.  -> (clones of out and info [and the index] as numpy)."""
    import torch

    pix = step.decoy.clone()
    torch.cuda.synchronize()
    t0, t1, t2 = _events(3)
    with torch.cuda.stream(S):   # warm run, on the decoy: a join that is lost later leaves the decoy's streams in `out`
        t0.record()
        out, info = step.call(c, pix)
        t1.record()
        S.synchronize()
        call_ms = t0.elapsed_time(t1)
        ix = c.set_encode_index(step.n, device=True) if index else None
        t0.record()
        delay.queue(_delay_for(call_ms))
        t1.record()
        pix.copy_(step.real)
        step.call(c, pix, out, info)
        pix.copy_(step.decoy2)
        got = [out.clone(), info.clone()] + ([ix.clone()] if index else [])
    S.synchronize()
    _conclusive(step.what, t0.elapsed_time(t1), call_ms)
    return _to_host(got)


@pytest.mark.parametrize("case", list(ENCODE_CASES))
def test_encode_waits_for_the_producer_and_joins_before_the_consumer(case, delay):
    """On a context's own non-default stream, with no synchronisation: delay, pixels copied over a decoy, the encode,
    pixels overwritten, outputs cloned.  The clones hold the oracle's streams and records of the real pictures."""
    import torch

    depth, geom, n = ENCODE_CASES[case]
    S = torch.cuda.Stream()
    c = _context_on(S)
    try:
        step = _Enc(c.device, depth, geom, n)
        step.check(_encode_behind_delay(delay, step, c, S))
    finally:
        c.close()


def test_encode_index_is_written_behind_the_same_fork_and_join(delay):
    """set_encode_index(device=True) at n = 130: the cloned indices equal those of a plain, synchronised run."""
    import torch

    import dwt_amd

    S = torch.cuda.Stream()
    c = _context_on(S)
    try:
        step = _Enc(c.device, 8, WIDE, 130)
        with torch.cuda.stream(S):
            plain_ix = c.set_encode_index(step.n, device=True)
            step.call(c, step.real)
            S.synchronize()
            plain = plain_ix.cpu().numpy()
        try:
            kept = _encode_behind_delay(delay, step, c, S, index=True)
        finally:
            c.set_encode_index()
        step.check(kept)
        for i in range(step.n):
            a, b = dwt_amd.index_from_row(plain[i].tobytes()), dwt_amd.index_from_row(kept[2][i].tobytes())
            assert 0 < a.nsegs <= dwt_amd.INDEX_MAX_SEGS and a.magic == dwt_amd.INDEX_MAGIC, i
            k = HEAD + 32 * a.nsegs
            assert bytes(b)[:k] == bytes(a)[:k], f"index of image {i}: {_first_diff(np.frombuffer(bytes(b)[:k], np.uint8), np.frombuffer(bytes(a)[:k], np.uint8))}"
    finally:
        c.close()


# ---- 2. the same for the decoder ------------------------------------------------------------------------------------

DECODE_CASES = {   # depth, geometry, n: one part below 4 streams, two below 24, four from there on
    "wide8_n3": (8, WIDE, 3), "odd8_n8": (8, ODD, 8), "wide8_n30": (8, WIDE, 30),
    "odd16_n3": (16, ODD, 3), "wide16_n8": (16, WIDE, 8), "odd16_n30": (16, ODD, 30),
}


def _decode_behind_delay(delay, step, c, S, before_call=None):
    import torch

    rows, lens, buf = step.decoy_rows.clone(), step.decoy_lens.clone(), step.buf0.clone()
    warm_rows, warm_lens, warm_buf = step.rows.clone(), step.lens.clone(), step.buf0.clone()
    torch.cuda.synchronize()
    t0, t1 = _events(2)
    with torch.cuda.stream(S):
        step.call(c, warm_rows, warm_lens, warm_buf)   # (cold: streams, events and scratch are made here)
        t0.record()
        step.call(c, warm_rows, warm_lens, warm_buf)
        t1.record()
        S.synchronize()
        call_ms = t0.elapsed_time(t1)
        if before_call:
            before_call()
        t0.record()
        delay.queue(_delay_for(call_ms))
        t1.record()
        rows.copy_(step.rows)
        lens.copy_(step.lens)
        step.call(c, rows, lens, buf)
        rows.copy_(step.decoy2_rows)
        lens.copy_(step.decoy2_lens)
        got = buf.clone()
    S.synchronize()
    _conclusive(step.what, t0.elapsed_time(t1), call_ms)
    return _to_host([got])


@pytest.mark.parametrize("case", list(DECODE_CASES))
def test_decode_waits_for_the_producer_and_joins_before_the_consumer(case, delay):
    """Stream rows and lengths are filled on S behind the delay (over valid decoy streams), decoded, overwritten with
    other valid streams right after the call returns, and the pixels cloned on S: the oracle's pictures, and every
    sentinel around the picture slots untouched."""
    import torch

    depth, geom, n = DECODE_CASES[case]
    S = torch.cuda.Stream()
    c = _context_on(S)
    try:
        step = _Dec(c.device, depth, geom, n)
        step.check(_decode_behind_delay(delay, step, c, S))
    finally:
        c.close()


def test_decode_with_offered_indices_behind_the_delay(delay):
    """Whole streams with the sidecar indices an earlier decode made, and no fallback to the serial walk: a part that
    read the decoy streams would turn its index down, which is an error then."""
    import torch

    S = torch.cuda.Stream()
    c = _context_on(S)
    try:
        step = _Dec(c.device, 8, WIDE, 8, whole=True)
        made = c.set_index(None, step.n)
        with torch.cuda.stream(S):
            step.call(c, step.rows, step.lens, step.buf0.clone())
        S.synchronize()
        assert all(made[i].nsegs > 0 for i in range(step.n))

        def offer():
            c.set_option("no_index_fallback", 1)
            c.set_index(made, 0)

        try:
            step.check(_decode_behind_delay(delay, step, c, S, before_call=offer))
        finally:
            c.set_index()
    finally:
        c.close()


# ---- 3. calls in flight behind one another, with scratch that grows --------------------------------------------------

def _sequence(dev):
    return [_Enc(dev, 8, (64, 48, 1), 2), _Enc(dev, 8, (512, 384, 3), 6), _Dec(dev, 8, (131, 77, 3), 3), _Enc(dev, 16, (256, 200, 3), 4),
            _Enc(dev, 8, WIDE, 130), _Dec(dev, 8, WIDE, 30, whole=True), _Chain(dev, ODD, 2)]


def test_calls_in_flight_with_growing_scratch_forward_and_reverse(delay):
    """Seven calls of changing geometry queued behind one delay on a fresh context (every scratch slot starts empty and
    grows under queued work; the encoder's part contexts appear mid-sequence), inputs overwritten after each call,
    one synchronisation at the end.  Then the reverse order on a second fresh context: grow-only scratch serves small
    geometries after large ones."""
    import torch

    dev = torch.device("cuda", 0)
    steps = _sequence(dev)
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    warm = _context_on(S)
    try:
        _run(S, warm, steps)
        _, _, call_ms = _run(S, warm, steps)
    finally:
        warm.close()
    results = []
    for order in (steps, steps[::-1]):
        c = _context_on(S)
        try:
            kept, delay_ms, _ = _run(S, c, order, delay, _delay_for(call_ms))
        finally:
            c.close()
        _conclusive("the sequence " + ("forward" if order is steps else "reversed"), delay_ms, call_ms)
        for st, k in zip(order, kept):
            st.check(k)
        results.append(kept if order is steps else kept[::-1])
    for st, a, b in zip(steps, *results):
        for x, y in zip(st.results(a), st.results(b)):
            assert (x == y).all(), f"{st.what}: forward and reversed runs differ: {_first_diff(x, y)}"


# ---- 4. two contexts, two streams, interleaved ----------------------------------------------------------------------

def test_two_contexts_interleaved_from_one_thread():
    """A encodes 130 pictures (twice), B decodes 30 streams and runs a deep round trip, on streams and geometries of their
    own; the calls alternate A, B, A, B with no synchronisation until the end.  The oracle's results, and the same as
    each context gives alone."""
    import torch

    dev = torch.device("cuda", 0)
    a_steps = [_Enc(dev, 8, WIDE, 130), _Enc(dev, 8, WIDE, 130, shift=2)]
    b_steps = [_Dec(dev, 8, ODD, 30), _RoundTrip16(dev, ODD, 3)]
    torch.cuda.synchronize()
    SA, SB = torch.cuda.Stream(), torch.cuda.Stream()
    A, B = _context_on(SA), _context_on(SB)
    try:
        alone_a, _, _ = _run(SA, A, a_steps)
        alone_b, _, _ = _run(SB, B, b_steps)
        kept_a, kept_b = [], []
        for a, b in zip(a_steps, b_steps):
            with torch.cuda.stream(SA):
                kept_a.append(a.queue(A))
            with torch.cuda.stream(SB):
                kept_b.append(b.queue(B))
        SA.synchronize()
        SB.synchronize()
        kept_a, kept_b = [_to_host(k) for k in kept_a], [_to_host(k) for k in kept_b]
    finally:
        A.close()
        B.close()
    for steps, kept, alone in ((a_steps, kept_a, alone_a), (b_steps, kept_b, alone_b)):
        for st, k, al in zip(steps, kept, alone):
            st.check(k)
            st.check(al)
            for x, y in zip(st.results(k), st.results(al)):
                assert (x == y).all(), f"{st.what}: interleaved and alone differ: {_first_diff(x, y)}"


# ---- 5. one context per host thread ---------------------------------------------------------------------------------

GEOMS = [WIDE, ODD, (64, 48, 1)]


def _host_encode(c, depth, pics, alloc):
    """dwtx_encode_images / dwtx_encode_images16 with buffers from alloc(bytes) -> list of streams."""
    arr = np.stack(pics)
    n, H, W, Cn = arr.shape
    sym, bound = ("dwtx_encode_images", c.lib.dwtx_encode_bound) if depth == 8 else ("dwtx_encode_images16", c.lib.dwtx_encode_bound16)
    stride = bound(W, H, Cn)
    src, dst = alloc(arr.nbytes), alloc(n * stride)
    src[:] = arr.reshape(-1).view(np.uint8)
    lens = (C.c_size_t * n)()
    rc = getattr(c.lib, sym)(c.h, src.ctypes.data, W, H, Cn, n, 0, dst.ctypes.data, stride, C.cast(lens, C.c_void_p), None)
    assert rc == 0, (sym, rc, c.lib.dwtx_last_error())
    return [dst[i * stride:i * stride + lens[i]].tobytes() for i in range(n)]


def _host_decode(c, depth, rows, geom, alloc):
    """dwtx_decode_images / dwtx_decode_images16 with buffers from alloc(bytes) -> list of pictures."""
    W, H, Cn = geom
    n = len(rows)
    stride = _r8(max(len(r) for r in rows) + 64)
    src = alloc(n * stride)
    src[:] = 0
    for i, r in enumerate(rows):
        src[i * stride:i * stride + len(r)] = np.frombuffer(r, dtype=np.uint8)
    lens = (C.c_size_t * n)(*[len(r) for r in rows])
    pstride = W * H * Cn
    dst = alloc(n * pstride * (1 if depth == 8 else 2))
    ow, oh, oc = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    head = (c.h, src.ctypes.data, stride, C.cast(lens, C.c_void_p), n, -1, dst.ctypes.data, pstride)
    if depth == 8:
        rc = c.lib.dwtx_decode_images(*head, ow, oh, oc)
    else:
        rc = c.lib.dwtx_decode_images16(*head, M16, ow, oh, oc, None)
    assert rc == 0, (depth, rc, c.lib.dwtx_last_error())
    pix = dst.view(_np_dtype(depth))
    return [pix[i * pstride:i * pstride + ow[i] * oh[i] * oc[i]].reshape(oh[i], ow[i], oc[i]).copy() for i in range(n)]


def _plan(seed, dev):
    """About 20 mixed calls for one thread: (kind, arguments, expected).  Device calls are steps, staged here; the
    host-buffer calls carry what the oracle gives.  Everything the oracle computes is computed here, before the threads
    start."""
    rng = np.random.default_rng(seed)

    def host_enc(depth, pinned):
        W, H, Cn = GEOMS[int(rng.integers(len(GEOMS)))]
        n, shift = int(rng.integers(2, 6)), int(rng.integers(POOL))
        pool, enc = _pool(depth, W, H, Cn), _streams(depth, W, H, Cn)
        return ("host_enc", (depth, [pool[(i + shift) % POOL] for i in range(n)], pinned), [enc[(i + shift) % POOL][0] for i in range(n)])

    def host_dec(depth, pinned, kind="host_dec", whole=False):
        geom = GEOMS[int(rng.integers(len(GEOMS)))]
        W, H, Cn = geom
        n, shift = int(rng.integers(2, 6)), int(rng.integers(POOL))
        which = [((i + shift) % POOL, len(_streams(depth, W, H, Cn)[(i + shift) % POOL][0])) if whole or i == 0 else _row_of(depth, W, H, Cn, i, shift)
                 for i in range(n)]   # (the whole stream first: the host call reads row 0's header)
        rows = [_streams(depth, W, H, Cn)[k][0][:L] for k, L in which]
        return (kind, (depth, rows, geom, pinned), [_decoded(depth, W, H, Cn, k, L) for k, L in which])

    def dev_step():
        depth = (8, 16)[int(rng.integers(2))]
        geom = GEOMS[int(rng.integers(len(GEOMS)))]
        n, shift = int(rng.integers(2, 9)), int(rng.integers(POOL))
        step = _Enc(dev, depth, geom, n, shift) if rng.integers(2) else _Dec(dev, depth, geom, n, shift)
        return ("step", step, None)

    plan = [host_enc(8, False), host_enc(16, True), host_enc(8, True), host_enc(16, False),
            host_dec(8, False), host_dec(16, True), host_dec(8, True), host_dec(16, False),
            host_dec(8, False, "index_dec", whole=True),
            ("step", _Enc(dev, 16, WIDE, 4, seed), None), ("step", _Dec(dev, 8, ODD, 5, seed), None),
            ("step", _Enc(dev, 8, (64, 48, 1), 3, seed), None), ("step", _Dec(dev, 16, WIDE, 8, seed), None)]
    plan += [dev_step() for _ in range(7)]
    return [plan[i] for i in rng.permutation(len(plan))]


def _failing_calls(c):
    """Calls that must fail with DWTX_ERR_ARG -> the messages they leave in this thread's dwtx_last_error()."""
    import torch

    msgs = []
    data = _streams(16, 64, 48, 1)[0][0]
    try:
        c.decode16(data, 0)
        msgs.append(b"decode16 with maxval 0 did not fail")
    except Exception as e:
        assert getattr(e, "rc", None) == ERR_ARG, e
        msgs.append(c.lib.dwtx_last_error())
    W, H, Cn = WIDE
    pix = _device_pixels(c.device, 8, W, H, Cn, 1, 0)
    pyr, r16, mask = c.transformation_fwd_pixels(pix)
    out = torch.empty_like(pix)
    wrong = mask ^ (1 << 14) or (1 << 14)
    rc = c.lib.dwtx_transformation_inv_pixels(c.h, out.data_ptr(), pyr.data_ptr(), r16.data_ptr(), wrong, W, H, Cn, 1)
    assert rc == ERR_ARG, rc
    msgs.append(c.lib.dwtx_last_error())
    return msgs


def _thread_body(tid, S, plan, fails, failed, results):
    import torch

    import dwt_amd

    lib = dwt_amd._lib.load()
    res = results[tid]
    res["error_before"] = lib.dwtx_last_error()
    with torch.cuda.stream(S):
        c = dwt_amd.Context(0)   # on torch's current stream: S
        pinned = []
        try:
            assert lib.dwtx_stream(c.h) == S.cuda_stream

            def pageable(nbytes):
                return np.empty(nbytes, dtype=np.uint8)

            def page_locked(nbytes):
                p = lib.dwtx_host_alloc(c.h, nbytes)
                assert p, lib.dwtx_last_error()
                pinned.append(p)
                return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p))

            got = []
            for pos, (kind, args, _) in enumerate(plan):
                if fails and pos == len(plan) // 2:
                    res["fail_msgs"] = _failing_calls(c)
                    failed.set()
                if kind == "step":
                    got.append(args.queue(c))
                elif kind == "host_enc":
                    depth, pics, pin = args
                    got.append(_host_encode(c, depth, pics, page_locked if pin else pageable))
                elif kind == "host_dec":
                    depth, rows, geom, pin = args
                    got.append(_host_decode(c, depth, rows, geom, page_locked if pin else pageable))
                else:   # index_dec: a decode that makes the indices, then one that is offered them and may not fall back
                    depth, rows, geom, pin = args
                    made = c.set_index(None, len(rows))
                    first = _host_decode(c, depth, rows, geom, pageable)
                    assert all(made[i].nsegs > 0 for i in range(len(rows)))
                    c.set_option("no_index_fallback", 1)
                    c.set_index(made, 0)
                    second = _host_decode(c, depth, rows, geom, pageable)
                    c.set_index()
                    c.set_option("no_index_fallback", 0)
                    got.append((first, second))
            S.synchronize()
            res["got"] = [_to_host(g) if kind == "step" else g for g, (kind, _, _) in zip(got, plan)]
            if not fails:   # (the other thread has set the event, or has ended: see the `finally` of _thread)
                failed.wait()
                res["error_after"] = lib.dwtx_last_error()
        finally:
            for p in pinned:
                lib.dwtx_host_free(c.h, p)
            c.close()


def _thread(tid, S, plan, fails, failed, results):
    try:
        _thread_body(tid, S, plan, fails, failed, results)
    except BaseException as e:   # an exception in a thread fails the test (the main thread raises it after join)
        results[tid]["exception"] = e
    finally:
        if fails:
            failed.set()


def test_one_context_per_host_thread():
    """Two threads, each with its own context on its own stream, run about 20 mixed calls at once (ctypes releases the
    GIL): device and host-buffer encodes and decodes, pageable and page-locked buffers, 8-bit and deep pictures,
    changing geometries, a sidecar-index decode.  One thread also makes calls that must fail; the other's
    dwtx_last_error() never shows their messages."""
    import torch

    dev = torch.device("cuda", 0)
    plans = [_plan(101, dev), _plan(202, dev)]
    _streams(16, 64, 48, 1), _pool(8, *WIDE)   # what _failing_calls reads: the oracle is not asked from a thread
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results = [{}, {}]
    failed = threading.Event()
    threads = [threading.Thread(target=_thread, args=(t, streams[t], plans[t], t == 0, failed, results)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(2):
        if "exception" in results[t]:
            raise results[t]["exception"]
    for t in range(2):
        assert len(results[t]["got"]) == len(plans[t]) >= 20
        for pos, ((kind, args, want), got) in enumerate(zip(plans[t], results[t]["got"])):
            where = f"thread {t} call {pos} ({kind})"
            if kind == "step":
                args.check(got)
            elif kind == "host_enc":
                assert got == want, where
            else:
                for g in (got if kind == "index_dec" else (got,)):
                    assert len(g) == len(want), where
                    for a, b in zip(g, want):
                        assert b is not None and a.shape == b.shape and (a == b).all(), where
    msgs = results[0]["fail_msgs"]
    print("messages of the failing calls:", msgs)
    assert msgs[0] == b"maxval 0 is outside 1..65535"
    assert msgs[1].startswith(b"levels16 mask "), msgs[1]
    assert results[0]["error_before"] == b"" and results[1]["error_before"] == b""
    assert results[1]["error_after"] == b"", "the failing thread's message showed up in the other thread"


# ---- 6. dwtx_ctx_create and dwtx_stream ------------------------------------------------------------------------------

def test_a_context_with_its_own_stream_chained_through_dwtx_stream(delay):
    """The producer runs on a torch stream P, the context on the stream dwtx_ctx_create made: events on dwtx_stream()
    order the two, in both directions."""
    import torch

    P = torch.cuda.Stream()
    c = _context_with_own_stream()
    try:
        handle = c.lib.dwtx_stream(c.h)
        assert handle and handle != P.cuda_stream
        CS = torch.cuda.ExternalStream(handle)
        step = _Enc(c.device, 8, WIDE, 130)
        pix = step.decoy.clone()
        torch.cuda.synchronize()
        t0, t1 = _events(2)
        with torch.cuda.stream(CS):   # warm run on the decoy
            t0.record()
            out, info = step.call(c, pix)
            t1.record()
        CS.synchronize()
        call_ms = t0.elapsed_time(t1)
        ready, encoded = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(P):
            t0.record()
            delay.queue(_delay_for(call_ms))
            t1.record()
            pix.copy_(step.real)
            ready.record()
        CS.wait_event(ready)
        step.call(c, pix, out, info)
        encoded.record(CS)
        with torch.cuda.stream(P):
            P.wait_event(encoded)
            got = [out.clone(), info.clone()]
            pix.copy_(step.decoy2)
        P.synchronize()
        _conclusive(step.what + " on dwtx_stream()", t0.elapsed_time(t1), call_ms)
        step.check(_to_host(got))
        c.sync()
    finally:
        c.close()
    S = torch.cuda.Stream()
    c = _context_on(S)
    try:
        assert c.lib.dwtx_stream(c.h) == S.cuda_stream
    finally:
        c.close()


# ---- 7. teardown with work queued -----------------------------------------------------------------------------------

def test_destroy_with_an_encode_queued(delay):
    """dwtx_ctx_destroy right behind a delay and a four-part encode: the caller's output tensors hold the oracle's bytes."""
    import torch

    S, other = torch.cuda.Stream(), torch.cuda.Stream()
    step = _Enc(torch.device("cuda", 0), 8, WIDE, 130)
    warm = _context_on(S)
    try:
        _run(S, warm, [step])
        _, _, call_ms = _run(S, warm, [step])
    finally:
        warm.close()
    c = _context_on(S)
    t0, t1 = _events(2)
    try:
        with torch.cuda.stream(S):
            t0.record()
            delay.queue(_delay_for(call_ms))
            t1.record()
            kept = step.queue(c)
    finally:
        c.close()   # dwtx_ctx_destroy, at once
    torch.cuda.synchronize()
    _conclusive(step.what + " before dwtx_ctx_destroy", t0.elapsed_time(t1), call_ms)
    with torch.cuda.stream(other):
        got = [kept[0].clone(), kept[1].clone()]
    other.synchronize()
    step.check(_to_host(got))


def test_free_waits_for_the_call_that_reads_the_buffer(delay):
    """dwtx_free of a dwtx_malloc buffer that a queued encode still reads returns only after that encode."""
    import torch

    S = torch.cuda.Stream()
    c = _context_on(S)
    try:
        step = _Enc(c.device, 8, WIDE, 130)
        with torch.cuda.stream(S):
            t0, t1 = _events(2)
            step.call(c, step.real)   # (cold)
            t0.record()
            out, info = step.call(c, step.decoy)
            t1.record()
            S.synchronize()
            call_ms = t0.elapsed_time(t1)
            host = step.real.cpu().numpy()
            buf = c.lib.dwtx_malloc(c.h, host.nbytes)
            assert buf, c.lib.dwtx_last_error()
            assert c.lib.dwtx_upload(c.h, buf, host.ctypes.data, host.nbytes) == 0
            W, H, Cn = step.geom
            after = torch.cuda.Event()
            t0.record()
            delay.queue(_delay_for(call_ms))
            t1.record()
            rc = c.lib.dwtx_encode_device(c.h, buf, W, H, Cn, step.n, 0, out.data_ptr(), out.shape[1], info.data_ptr())
            after.record()
            c.lib.dwtx_free(c.h, buf)
            over = after.query()
            assert rc == 0, c.lib.dwtx_last_error()
        S.synchronize()
        _conclusive(step.what + " from a dwtx_malloc buffer", t0.elapsed_time(t1), call_ms)
        assert over, "dwtx_free returned while the encode that reads the buffer was still queued"
        step.check(_to_host([out, info]))
    finally:
        c.close()


def test_twenty_contexts_come_and_go(ctx):
    """Twenty contexts, each of which ran a four-part encode and a four-part decode (so each made its side streams,
    events and part contexts), are destroyed; the session's context then still gives the oracle's bytes."""
    import torch

    dev = torch.device("cuda", 0)
    steps = [_Enc(dev, 8, WIDE, 130), _Dec(dev, 8, WIDE, 30)]
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    for _ in range(20):
        c = _context_on(S)
        try:
            kept, _, _ = _run(S, c, steps)
        finally:
            c.close()
        for st, k in zip(steps, kept):
            st.check(k)
    W, H, Cn = ODD
    pics = _pool(8, W, H, Cn)[:2]
    out, info = ctx.encode_device(torch.from_numpy(np.stack(pics)).to(ctx.device))
    _check_streams(out.cpu().numpy(), info.cpu().numpy(), 8, W, H, Cn, 0, "the session's context afterwards")
