"""GPU: a call's result must not depend on what its context decoded or encoded before.

A context keeps 25 grow-only scratch slots across calls and clears almost none of them ("What survives a
call"): each table stays dirty under an invariant of the form "every word this call reads, this call wrote".  The other
files cannot see a violation — they decode the same streams again under another switch on the session's context, so a
word that is not written, or a clear that is missing, reads the right answer from the run before.  Here the history is
chosen: every case is `run_history` (tests/history.py: noise or flat pictures of other seeds, through the decoder, the
16-bit decoder, the encoder, a crop route, a reduced or an indexed decode — tests/test_history_cpu.py holds each to the
conditions that make its stale words wrong ones) on a private context, then ONE target call whose entire result must be
the oracle's: the whole destination buffer with the pattern outside the pictures, the decode records, and for encodes
the streams, their records and the sidecar index.  One fixture gives a context that has run nothing.

Checked once with two builds that break an invariant in values only (profiles/history_mutants.txt has the argument and the
counts, also of tests/test_unpack_gpu.py, test_codec_gpu.py, test_count_skip_gpu.py and test_crop_gpu.py): without the
root-image clear of DecodeCall::queue_clears (unpack.hip; the root image is only ever a coefficient: read_preamble stores
it, k_root_copy copies it, the lifting reads it) 217 of the 514 cases here fail — the targets with a channel whose root
image is all zeros, sparse and mixed batches, after every history and as a fresh context's first call — against 1 of 49, 0
of 115, 2 of 19 and 0 of 111 in the older files; with a k_apply_all that does not store the tiles in which nothing becomes
significant 321 fail, every switch of the sweep and both crop routes among them (older files: 12, 42, 13 and 23)."""
import numpy as np
import pytest

import floats
import history as Hs
import orc
import test_crop_gpu as CR
import test_encode_index_gpu as EI
import test_float_gpu as F
import test_planar_gpu as P
import test_views_gpu as V

pytestmark = pytest.mark.gpu


class Opts:
    """tests/conftest.py's `opts` for a context of one's own: switches set with set_option, put back by restore()"""

    def __init__(self, c):
        self.c, self.used = c, []

    def set(self, name, value=1):
        self.used.append(name)
        self.c.set_option(name, value)

    def restore(self):
        for name in self.used:
            self.c.set_option(name, 0)


@pytest.fixture(scope="module")
def own(ctx):
    """A context whose history these tests alone write (it depends on `ctx`: no GPU, no test)"""
    import dwt_amd

    c = dwt_amd.Context(0)
    yield c
    c.close()


@pytest.fixture
def fresh(ctx):
    """A context that has run nothing yet"""
    import dwt_amd

    c = dwt_amd.Context(0)
    yield c
    c.close()


# ---- the target calls ------------------------------------------------------------------------------------------------------

def check_infos(infos, rows, W, H, Cn, pixels_max):
    """the decode records against orc.decode_stage (tests/test_count_skip_gpu.py both_ways, tests/test_levels_gpu.py check_dense)"""
    for i, (I, r) in enumerate(zip(infos, rows)):
        ref = orc.decode_stage(r, W, H, Cn, pixels_max)
        if ref is None:
            assert I.status == 1, i
            continue
        _, level, missing, planes = ref
        assert I.status == 0 and I.level == level and list(I.missing) == missing.tolist() and list(I.planes)[:Cn] == planes, (i, I.status, I.level, level)
        assert (I.truncated & 1) == int((missing > 0).any()), (i, I.truncated)   # (a flat picture's one segment leaves missing[0] at -1)


def layout_of(sink, t):
    if sink == "nchw" or (sink == "fp16" and t.Cn == 3):
        return P.nchw(t.W, t.H, n=t.n)
    return V.grid(t.W, t.H, t.Cn, rows=1, cols=t.n)


def check_dense(c, t, rows, pixels_max):
    """dwtx_decode_device / dwtx_decode_device16 into a patterned buffer of dense slots: the oracle's picture in a slot's first
    ow * oh * C samples, the pattern in every other sample — all of an unreadable stream's slot"""
    import deep

    size = t.W * t.H * t.Cn
    before = V.pattern(t.n * size + 64, t.is16)
    want = before.copy()
    for i, r in enumerate(rows):
        ref = V.oracle_decode(r, t.W, t.H, t.Cn, t.is16, pixels_max)
        if ref is not None:
            want[i * size:i * size + ref.size] = ref.reshape(-1)
    streams, lens = F.upload(c, rows)
    buf = V.to_device(c, before)
    out = buf[:t.n * size].view(t.n, size)
    lm = deep.levels_max(t.W, t.H, pixels_max)
    if t.is16:
        _, infos = c.decode_device16(streams, lens, t.W, t.H, t.Cn, V.M16, levels_max=lm, out=out)
    else:
        _, infos = c.decode_device(streams, lens, t.W, t.H, t.Cn, levels_max=lm, out=out)
    c.sync()
    got = V.to_host(buf, t.is16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} samples differ, first at {bad[:5]} (slots of {size}): got {got[bad[:5]]}, want {want[bad[:5]]}"
    return infos


def check_decode_target(c, opts, s):
    t, rows, pixels_max = s.target, list(Hs.rows_of(s.target)), Hs.pixels_max_of(s.target)
    W, H, Cn = t.W, t.H, t.Cn
    maxval = V.M16 if t.is16 else 255
    if s.sink == "dense":
        infos = check_dense(c, t, rows, pixels_max)
    elif s.sink in ("grid", "nchw"):
        infos = V.check_decode(c, layout_of(s.sink, t), W, H, Cn, t.is16, rows, pixels_max)
    elif s.sink == "fp16":
        scale, bias = floats.SETS["imagenet"](maxval)
        F.check_float(c, layout_of(s.sink, t), W, H, Cn, rows, "float16", maxval, scale, bias, pixels_max)
        return
    elif s.sink in ("crop1", "crop2"):
        cw, ch = W // 2 + 3, H // 2 + 2
        origins = [((W - cw) * i // (t.n - 1), (H - ch) * (t.n - 1 - i) // (t.n - 1)) for i in range(t.n)]   # both far corners, odd ones between
        infos = CR.check_crop(c, opts, V.stack(cw, ch, Cn, n=t.n), W, H, Cn, t.is16, rows, origins, pixels_max, routes=(int(s.sink[-1]),))
    else:
        assert s.sink == "index"
        import dwt_amd

        made = EI._decoder_made(c, rows, W, H, Cn)[0]   # (this context's own serial walk wrote them — before the dirt)
        assert all(m.magic == dwt_amd.INDEX_MAGIC and m.nsegs > 0 for m in made)
        Hs.run_history(c, Hs.calls_of(s))
        c.set_index(made, 0)
        opts.set("no_index_fallback", 1)   # a correct index is accepted: the indexed walk is the one that runs
        try:
            infos = check_dense(c, t, rows, pixels_max)
        finally:
            c.set_index()
    check_infos(infos, rows, W, H, Cn, pixels_max)


def check_encode_target(c, ctx, s):
    """dwtx_encode_device (or dwtx_encode_view_float of the same samples as float32 and float16) with a sidecar index wanted:
    streams and records against orc.encode; the index of a whole stream against the one the session context's serial walk
    makes of the oracle's stream (tests/test_encode_index_gpu.py's yardstick), of a flat or capacity-cut one its header alone"""
    import torch

    t = s.target
    pics, capacity = Hs.encoder_pictures(t.W, t.H, t.Cn, t.content)
    wants = [orc.encode(p, capacity) for p in pics]
    whole = [orc.encode(p)[0] for p in pics]
    pix = torch.from_numpy(np.stack(pics)).to(c.device)
    sources = [pix] if s.sink == "encode" else [pix.float(), pix.half()]
    for src in sources:
        dev_index = c.set_encode_index(len(pics), device=True)
        try:
            out, info = c.encode_device(src, capacity) if s.sink == "encode" else c.encode_view_float(src, maxval=255, capacity=capacity)
            enc = EI._rows(c, dev_index)
        finally:
            c.set_encode_index()
        infos, host = V.infos_of(info), out.cpu().numpy()
        indexed = []
        for i, (want, st) in enumerate(wants):
            I = infos[i]
            assert I.error == 0, i
            assert host[i, :I.nbytes].tobytes() == want, i
            assert list(I.planes)[:t.Cn] == list(st.planes)[:t.Cn] and (I.root_bits, I.total_bits) == (st.root_bits, st.total_bits), i
            if max(st.planes[:t.Cn]) == 0 or want != whole[i]:
                EI._header_only(enc[i], t.W, t.H, t.Cn)
            else:
                indexed.append(i)
        if indexed:
            made = EI._decoder_made(ctx, [whole[i] for i in indexed], t.W, t.H, t.Cn)[0]
            EI._assert_equal([enc[i] for i in indexed], list(made), s.name)


def run(c, ctx, s):
    opts = Opts(c)
    try:
        if s.switch:
            opts.set(*s.switch)
        if s.sink != "index":   # (which makes its indices first)
            Hs.run_history(c, Hs.calls_of(s))
        if s.sink.startswith("encode"):
            check_encode_target(c, ctx, s)
        else:
            check_decode_target(c, opts, s)
    finally:
        opts.restore()


def cases(group, with_history):
    sel = [s for s in Hs.group(group) if (s.hist != "none") == with_history]
    return pytest.mark.parametrize("s", sel, ids=Hs.ids(sel))


# ---- the tests ---------------------------------------------------------------------------------------------------------------

@cases("decode", True)
def test_a_plain_decode_after_every_history(own, ctx, s):
    """(a) noise, (b) 16-bit noise and bytes before a 16-bit sink, (c) the other channel count, (d) the transposed geometry,
    (e) an encode, (f) a crop, (g) a reduced decode, (h) an indexed one, (i) flat dirt before noise"""
    run(own, ctx, s)


@cases("decode", False)
def test_a_plain_decode_as_a_contexts_first_call(fresh, ctx, s):
    run(fresh, ctx, s)


@cases("switch", True)
def test_every_decoder_switch_after_a_decode_of_other_streams(own, ctx, s):
    run(own, ctx, s)


@cases("sink", True)
def test_every_sink_after_bytes_deep_pixels_and_before_a_broken_batch(own, ctx, s):
    run(own, ctx, s)


@cases("crop", True)
def test_a_crop_route_after_the_other_route_and_after_a_plain_decode(own, ctx, s):
    run(own, ctx, s)


@cases("crop", False)
def test_a_crop_as_a_contexts_first_call(fresh, ctx, s):
    run(fresh, ctx, s)


@cases("broken", True)
def test_reduced_stopped_cut_and_unreadable_streams_after_whole_noise(own, ctx, s):
    """rings the target never reaches hold dirt; the unreadable stream's slot keeps the pattern"""
    run(own, ctx, s)


@cases("broken", False)
def test_a_broken_batch_as_a_contexts_first_call(fresh, ctx, s):
    run(fresh, ctx, s)


@cases("index", True)
def test_a_target_that_is_offered_its_own_index(own, ctx, s):
    run(own, ctx, s)


@cases("encode", True)
def test_an_encode_after_an_encode_and_after_a_decode(own, ctx, s):
    run(own, ctx, s)


@cases("encode", False)
def test_an_encode_as_a_contexts_first_call(fresh, ctx, s):
    run(fresh, ctx, s)
