"""What a context decoded or encoded BEFORE a call — test infrastructure only, CPU only: the dirt, the targets and the
scenarios of tests/test_history_cpu.py and tests/test_history_gpu.py.

A context keeps its scratch slots from call to call and clears almost nothing of them ("What survives a call"):
every word a call reads it must have written itself.  A test that decodes the same streams twice cannot see a violation —
the stale word is the right answer.  Here every target call is preceded by calls that leave DIRT in the slots: pictures
that share next to no coefficient with the target (coincidence), that have more bit planes than it on every channel (so
every segment the target leaves empty was full before), and that are at least as large in every dimension a slot is sized
by (so nothing grows during the target call and the stale bytes are the dirt's, not a fresh allocation's).
tests/test_history_cpu.py holds every scenario to these three conditions with the oracle alone; the GPU file runs them.

Dirt is orc.synth's noise (kind 1) or a flat picture, with seeds from DIRT_SEED on; targets use seeds below 100.  (orc.synth's
kind 0 is unfit as dirt: 11 to 16 % of its coefficients are 0, which is what a target's unwritten coefficient would be.)"""
import collections
import functools

import numpy as np

import deep
import levels
import orc
import test_views_gpu as V

# (chosen: RGB noise laid over a gray target — history (c) — runs at 0.9 % because its Y plane is a mean of three channels, and
# seeds 9000 to 9600 put one pair or another of the smaller shapes past the cap; tests/test_history_cpu.py holds whatever stands here)
DIRT_SEED = 9700
DIRT_N = 8                     # images of a dirt call: two parts of four
COINCIDENCE_MAX = 0.01
DEEP_AMPLITUDE = {1: 28000, 3: 24000}   # noise in [0, A] needs 16 bit planes and no more (tests/test_history_cpu.py), maxval 65535
BRIGHT = 60                    # the one bright pixel: six bit planes, below every plane count of the noise


# ---- dirt ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dirt_picture(W, H, Cn, kind="noise", depth=8, i=0):
    """Picture i of a dirt batch.  kind: "noise" or "flat"; depth: 8 (bytes), 4095 or 65535 (uint16, that maxval)."""
    assert kind in ("noise", "flat") and depth in (8, 4095, 65535)
    if kind == "flat":
        v = 31 + 17 * i
        return np.full((H, W, Cn), v if depth == 8 else v * (depth // 255), dtype=np.uint8 if depth == 8 else np.uint16)
    if depth == 8:
        return orc.synth(W, H, Cn, DIRT_SEED + i, 1)
    return deep.noise(W, H, Cn, 4095 if depth == 4095 else DEEP_AMPLITUDE[Cn], seed=DIRT_SEED + i)


@functools.lru_cache(maxsize=None)
def dirt_stream(W, H, Cn, kind="noise", depth=8, i=0):
    p = dirt_picture(W, H, Cn, kind, depth, i)
    return (orc.encode(p) if depth == 8 else deep.deep_encode(p))[0]


def dirt_streams(W, H, Cn, n=DIRT_N, kind="noise", depth=8):
    """The dirt as whole streams of a batch"""
    return [dirt_stream(W, H, Cn, kind, depth, i) for i in range(n)]


def stride_of(rows):
    """The stream stride tests upload a batch with (tests/test_float_gpu.py upload())"""
    return (max(len(r) for r in rows) + 64 + 7) // 8 * 8


# ---- coincidence and plane counts ----------------------------------------------------------------------------------------------

def lin_of(pix):
    """The linearised coefficient planes [C, W*H] of a picture: orc.stage_dump for bytes, its stages for deep pixels"""
    if pix.dtype == np.uint8:
        return orc.stage_dump(pix)[1]
    return orc.linearize(orc.forward(deep.rgb2ycocg(pix) if pix.shape[2] == 3 else pix.astype(np.int32)))


def geometry_of(data):
    """(W, H, C) of a .dwt's header"""
    return (data[2] | (data[3] << 8)) + 1, (data[4] | (data[5] << 8)) + 1, 3 if data[1:2] == b"6" else 1


def coincidence(dirt_pix, target):
    """The share of positions of the linearised coefficient planes at which dirt and target hold the same value.  target: a
    picture, or a stream (whole or a prefix: what the oracle decodes of it, zeros where it decodes nothing; 0.0 for a stream
    it cannot read — nothing of it is written).  Planes of different geometries are laid over each other from their first
    coefficient on, as the slots lay them."""
    if isinstance(target, (bytes, bytearray)):
        if len(target) < 6:
            return 0.0
        r = orc.decode_stage(bytes(target), *geometry_of(target))
        if r is None:
            return 0.0
        t = r[0]
    else:
        t = lin_of(target)
    d, t = lin_of(dirt_pix).reshape(-1), t.reshape(-1)
    m = min(d.size, t.size)
    return float((d[:m] == t[:m]).mean())


@functools.lru_cache(maxsize=None)
def planes_of(data):
    """The plane counts a stream's preamble states, per channel; None: unreadable"""
    if len(data) < 6:
        return None
    r = orc.decode_stage(data, *geometry_of(data))
    return None if r is None else tuple(r[3])


# ---- history: the calls before the target ----------------------------------------------------------------------------------------

# how -> the family of slots the call fills ("decode": unpack.hip's and codec.hip's; "encode": pack.hip's and codec.hip's)
HOWS = {"decode": "decode", "decode16": "decode", "decode4095": "decode", "reduced": "decode", "indexed": "decode", "crop1": "decode",
        "crop2": "decode", "encode": "encode"}
DEPTH = {"decode16": 65535, "decode4095": 4095}

Call = collections.namedtuple("Call", "how W H Cn n kind stride")


def call(how, W, H, Cn, n=DIRT_N, kind="noise", stride=0):
    """One dirt call; stride: the least stream stride to upload its streams with (0: their own)"""
    assert how in HOWS
    rows = dirt_streams(W, H, Cn, n, kind, DEPTH.get(how, 8))
    return Call(how, W, H, Cn, n, kind, max(stride, stride_of(rows)))


def pictures_of(cl):
    return [dirt_picture(cl.W, cl.H, cl.Cn, cl.kind, DEPTH.get(cl.how, 8), i) for i in range(cl.n)]


def streams_of(cl):
    return dirt_streams(cl.W, cl.H, cl.Cn, cl.n, cl.kind, DEPTH.get(cl.how, 8))


def upload(c, rows, stride=0):
    """tests/test_float_gpu.py upload() with a least stride"""
    import torch

    stride = max(stride, stride_of(rows))
    host = np.full((len(rows), stride), 0xA5, dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return torch.from_numpy(host).to(c.device), torch.tensor([len(r) for r in rows], dtype=torch.int64, device=c.device)


def crop_of(W, H):
    """the dirt's crop: odd origin and sides (tests/test_crop_gpu.py general_crops)"""
    return W // 2 + 1, H // 2 + 1, (W // 3) | 1, (H // 3) | 1


def dirty(c, W, H, Cn, n, how, kind="noise", stride=0):
    """One call on context `c` that leaves dirt behind, then a sync.  how: "decode" (dwtx_decode_device of n noise streams),
    "decode16" / "decode4095" (dwtx_decode_device16 of deep noise, that maxval), "reduced" (a decode one level short,
    levels_max), "indexed" (a decode that collects the streams' indices and one that is offered them), "crop1" / "crop2"
    (dwtx_decode_view_crop under that route), "encode" (dwtx_encode_device of n noise pictures).  Nothing is asserted of the
    dirt's own result beyond status 0: the other test files own that."""
    import torch

    cl = call(how, W, H, Cn, n, kind, stride)
    if how == "encode":
        out, info = c.encode_device(torch.from_numpy(np.stack(pictures_of(cl))).to(c.device))
        c.sync()
        assert all(I.error == 0 for I in V.infos_of(info))
        return
    streams, lens = upload(c, streams_of(cl), cl.stride)
    if how in ("crop1", "crop2"):
        cw, ch, x0, y0 = crop_of(W, H)
        into = torch.zeros((n, ch, cw, Cn), dtype=torch.uint8, device=c.device)
        c.set_option("crop_route", int(how[-1]))
        try:
            infos = c.decode_view_crop(streams, lens, into, (W, H), (x0, y0))
        finally:
            c.set_option("crop_route", 0)
    elif how in DEPTH:
        infos = c.decode_device16(streams, lens, W, H, Cn, DEPTH[how])[1]
    elif how == "indexed":
        made = c.set_index(None, n)
        try:
            infos = c.decode_device(streams, lens, W, H, Cn)[1]
            c.set_index(made, 0)
            infos += c.decode_device(streams, lens, W, H, Cn)[1]
        finally:
            c.set_index()
    else:
        infos = c.decode_device(streams, lens, W, H, Cn, levels_max=levels.levels_of(W, H) - 1 if how == "reduced" else -1)[1]
    c.sync()
    assert all(I.status == 0 for I in infos)


def run_history(c, calls):
    for cl in calls:
        dirty(c, cl.W, cl.H, cl.Cn, cl.n, cl.how, cl.kind, cl.stride)


# ---- targets -------------------------------------------------------------------------------------------------------------------

# W, H, C: the smallest shapes the other files name as reaching each path
GENERAL_GRAY, GENERAL_RGB = (263, 135, 1), (263, 135, 3)   # general, odd, reduces to the wide 132x68
WIDE_GRAY = (256, 256, 1)                                  # 16-bit rings, the two-level kernel, square tiles
RING_EDGES = (260, 516, 1)                                 # tiles cut by ring edges
TAIL_RGB, TAIL_GRAY = (72, 68, 3), (64, 64, 1)             # 72x68: one wide level, then the LDS tail; 64x64: all tail
SHAPES = [GENERAL_GRAY, GENERAL_RGB, WIDE_GRAY, RING_EDGES, TAIL_RGB, TAIL_GRAY]
SWEPT = [GENERAL_RGB, WIDE_GRAY]

# content -> the batch's rows.  "synth": whole streams of orc.synth kind 0 (one uniform part: the fused route); "deep": whole
# streams of deep.smooth_noise (maxval 4095); "noise": whole streams of orc.synth kind 1, the targets' seeds; "mixed": a flat
# picture, one bright pixel, a whole stream, a cut one and one that stops a level early (parts that are finished image by
# image); "broken": whole, stopped, cut, unreadable (7 bytes), whole; "sparse": whole streams of one-bright-pixel pictures — a
# uniform part again, so the fused route, with tiles in which nothing ever becomes significant (orc.synth's pictures have
# none at most shapes)
CONTENTS = ("synth", "deep", "noise", "mixed", "broken", "sparse")

Target = collections.namedtuple("Target", "W H Cn n content is16 capped")


def target(shape, n, content="synth", is16=False, capped=False):
    """is16: the sink holds 16-bit samples (maxval 4095), whatever the streams were made of; capped: the call's levels_max
    is one level short of the whole picture"""
    assert content in CONTENTS and n in (3, 5)
    return Target(*shape, n, content, is16, capped)


def flat_picture(W, H, Cn, v=77):
    return np.full((H, W, Cn), v, dtype=np.uint8)


def bright_pixel(W, H, Cn, i=0):
    """black but for one pixel (picture i: its own place and value): nearly every tile of every ring is empty"""
    pix = np.zeros((H, W, Cn), dtype=np.uint8)
    pix[(H // 3 + 7 * i) % H, (W // 2 + 13 * i) % W] = BRIGHT - i
    return pix


def stopped(W, H, Cn, i):
    """picture i's stream, as far as the level before the last"""
    return levels.prefix_for_level(levels.stream(W, H, Cn, False, i), W, H, Cn, levels.levels_of(W, H) - 2)


@functools.lru_cache(maxsize=None)
def rows_of(t):
    """The target's streams, one per image"""
    W, H, Cn = t.W, t.H, t.Cn
    whole = lambda i: V.oracle_encode(W, H, Cn, False, i)[0]   # noqa: E731
    if t.content == "synth":
        rows = [whole(i) for i in range(t.n)]
    elif t.content == "deep":
        rows = [V.oracle_encode(W, H, Cn, True, i)[0] for i in range(t.n)]
    elif t.content == "noise":
        rows = [orc.encode(orc.synth(W, H, Cn, i, 1))[0] for i in range(t.n)]
    elif t.content == "sparse":
        rows = [orc.encode(bright_pixel(W, H, Cn, i))[0] for i in range(t.n)]
    elif t.content == "mixed":
        rows = [orc.encode(flat_picture(W, H, Cn))[0], orc.encode(bright_pixel(W, H, Cn))[0], whole(2), V.cut(*V.oracle_encode(W, H, Cn, False, 3)),
                stopped(W, H, Cn, 4)][:t.n]
    else:
        rows = [whole(0), stopped(W, H, Cn, 1), V.cut(*V.oracle_encode(W, H, Cn, False, 2)), whole(3)[:7], whole(4)][:t.n]
    return tuple(rows)


def pixels_max_of(t):
    return orc.geometry(t.W, t.H).pixels[levels.levels_of(t.W, t.H) - 1] if t.capped else -1


# what the encoder targets code: name -> (pictures, capacity)
@functools.lru_cache(maxsize=None)
def encoder_pictures(W, H, Cn, content):
    """"mixed": flat, one bright pixel and two of orc.synth kind 0, whole; "cut": three of kind 0 under a CAPACITY of 500 bytes"""
    if content == "mixed":
        return [flat_picture(W, H, Cn), bright_pixel(W, H, Cn), orc.synth(W, H, Cn, 1, 0), orc.synth(W, H, Cn, 2, 0), flat_picture(W, H, Cn, 0)], 0
    assert content == "cut"
    return [orc.synth(W, H, Cn, i, 0) for i in range(3)], 500


# ---- scenarios -----------------------------------------------------------------------------------------------------------------

# sink: how the target call is made and checked.  "dense": dwtx_decode_device (16-bit: dwtx_decode_device16); "grid": a u8 (u16)
# tile grid on the quad grid; "nchw": planar RGB; "fp16": float16 with scale and bias; "crop1" / "crop2": a crop under that
# route; "index": a plain decode that is offered the streams' own indices; "encode", "encode_float": the encoder
Scenario = collections.namedtuple("Scenario", "name hist family target sink switch")   # (its calls: calls_of(s), made when first asked for)


@functools.lru_cache(maxsize=None)
def history(name, t, family="decode"):
    """The calls of history `name` before target t (W, H, Cn, n, and its streams' stride).  Every history ends with the call it is
    named after; where that call alone would let a slot grow during the target call (another family, fewer samples), a noise
    call of the target's own geometry and family comes first, so that whatever stays stale is still dirt."""
    W, H, Cn = t.W, t.H, t.Cn
    stride = stride_of(rows_of(t)) if isinstance(t, Target) else 0
    plain = call("decode", W, H, Cn, stride=stride)
    enc = call("encode", W, H, Cn)
    if name == "none":
        return ()
    how, own = ("encode", enc) if family == "encode" else ("decode", plain)   # (c) and (d) in the target's own family
    table = {
        "a": [plain],
        "b16": [call("decode16", W, H, Cn, stride=stride)],
        "b4095": [call("decode4095", W, H, Cn, stride=stride)],
        "c": [call(how, W, H, 3, stride=stride)] + ([call(how, W, H, 1, stride=stride)] if Cn == 3 else []),
        "d": [own, call(how, H, W, Cn, stride=stride)],
        "e": [plain, enc],
        "crop1": [plain, call("crop1", W, H, Cn, stride=stride)],
        "crop2": [plain, call("crop2", W, H, Cn, stride=stride)],
        "reduced": [plain, call("reduced", W, H, Cn, stride=stride)],
        "indexed": [call("indexed", W, H, Cn, stride=stride)],
        "flat": [plain, call("decode", W, H, Cn, kind="flat", stride=stride)],
    }
    calls = table[name]
    if family == "encode" and name != "e":
        calls = [enc] + calls
    return tuple(calls)


def _scenarios():
    out = []

    def add(group, hist, t, sink="dense", switch=None, family="decode"):
        # RGB noise before a gray target lays its Y plane over the target's: a mean of three channels, narrower than the noise, 0.9 % of
        # it zeros.  Over the 4096 coefficients of 64x64 that share scatters past the cap for one seed or another: (c) runs at the three
        # larger gray shapes, and at 72x68 the other way round
        if hist == "c" and (t.W, t.H, t.Cn) == TAIL_GRAY:
            return
        name = "%s-%s-%dx%dx%d-n%d-%s%s%s-%s%s" % (group, hist, t.W, t.H, t.Cn, t.n, t.content, "-u16" if getattr(t, "is16", False) else "",
                                                  "-capped" if getattr(t, "capped", False) else "", sink,
                                                  "-%s=%d" % switch if switch else "")
        out.append((group, Scenario(name, hist, family, t, sink, switch)))

    # every history before a plain decode, at every shape: one uniform batch of three (one part, both path families) or five
    # (two parts), and the mixed batch with the other count
    for k, shape in enumerate(SHAPES):
        for hist in ("a", "b16", "b4095", "c", "d", "e", "crop1", "crop2", "reduced", "indexed", "none"):
            add("decode", hist, target(shape, 3 + 2 * (k & 1), "synth"))
            add("decode", hist, target(shape, 5 - 2 * (k & 1), "mixed"))
            add("decode", hist, target(shape, 3 + 2 * (k & 1), "sparse"), "grid" if k & 1 else "dense")
        # (i) flat dirt before noise: stale zero flags and empty bitmaps where ones are needed
        add("decode", "flat", target(shape, 5, "noise"))
        add("decode", "flat", target(shape, 3, "noise"), "grid")
    # (b) the reverse: bytes before a 16-bit sink
    for shape in (GENERAL_RGB, WIDE_GRAY):
        add("decode", "a", target(shape, 5, "synth", is16=True))
        add("decode", "a", target(shape, 3, "mixed", is16=True), "grid")
    # the switch sweep: each decoder switch after history (a)
    switches = [("count_every_plane", 0), ("count_every_plane", 1), ("decode_parts", 2), ("decode_parts", 4), ("one_stream", 1), ("two_families", 1),
                ("no_square_tiles", 1), ("no_fine16", 1), ("no_fused_levels", 1), ("lift_rows", 4), ("lift_rows", 64)]
    for shape in SWEPT:
        for sw in switches:
            add("switch", "a", target(shape, 5, "synth"), "grid", sw)
            add("switch", "a", target(shape, 5, "mixed"), "dense", sw)
            add("switch", "a", target(shape, 5, "sparse"), "grid", sw)
        for route in (1, 2):
            add("switch", "a", target(shape, 5, "synth"), "crop%d" % route)
            add("switch", "a", target(shape, 5, "mixed"), "crop%d" % route)
            add("switch", "a", target(shape, 5, "sparse"), "crop%d" % route)
    # the sinks under (a), (b) and (g)
    for shape in (GENERAL_GRAY, GENERAL_RGB, WIDE_GRAY, TAIL_RGB):
        sinks = ["dense", "grid", "fp16"] + (["nchw"] if shape[2] == 3 else [])
        for sink in sinks:
            add("sink", "a", target(shape, 3, "synth"), sink)
            add("sink", "b16", target(shape, 5, "synth"), sink)
            add("sink", "b16", target(shape, 3, "sparse"), sink)
            add("sink", "a", target(shape, 5, "broken"), sink)
        # u16: deep streams after deep dirt; a 16-bit sink of byte streams after bytes, and of a broken batch
        add("sink", "b16", target(shape, 3, "deep", is16=True), "grid")
        add("sink", "b4095", target(shape, 5, "deep", is16=True), "dense")
        add("sink", "b16", target(shape, 5, "deep", is16=True), "fp16")
        add("sink", "a", target(shape, 5, "broken", is16=True), "grid")
    # (f) crops: the other route, or a plain decode, before each route
    for shape in (GENERAL_RGB, WIDE_GRAY, TAIL_GRAY):
        for route in (1, 2):
            for hist in ("crop%d" % (3 - route), "a", "none"):
                add("crop", hist, target(shape, 3, "synth"), "crop%d" % route)
                add("crop", hist, target(shape, 5, "broken"), "crop%d" % route)
                add("crop", hist, target(shape, 5, "sparse"), "crop%d" % route)
    # (g) a whole noise batch before a batch of reduced, stopped, cut and unreadable streams, with and without a cap; and
    # reduced dirt before whole targets (in the first loop)
    for shape in SHAPES:
        for capped in (False, True):
            add("broken", "a", target(shape, 5, "broken", capped=capped))
            add("broken", "none", target(shape, 5, "broken", capped=capped))
        add("broken", "a", target(shape, 5, "synth", capped=True), "grid")
    # (h) a target that is offered its own index, after an indexed decode of other streams and after a plain one
    for shape in (GENERAL_RGB, WIDE_GRAY, RING_EDGES):
        for hist in ("indexed", "a"):
            add("index", hist, target(shape, 5, "synth"), "index")
            add("index", hist, target(shape, 5, "sparse"), "index")
    # the encoder, after an encode (e) and after a decode (a) of noise, after encodes of the other channel count (c) and of the
    # transposed geometry (d)
    for shape in (GENERAL_RGB, WIDE_GRAY, RING_EDGES, TAIL_GRAY):
        for hist in ("e", "a", "c", "d", "none"):
            for content, n in (("mixed", 5), ("cut", 3)):   # (encoder_pictures)
                add("encode", hist, EncTarget(*shape, n, content), "encode", family="encode")
            add("encode", hist, EncTarget(*shape, 5, "mixed"), "encode_float", family="encode")
    return out


EncTarget = collections.namedtuple("EncTarget", "W H Cn n content")
SCENARIOS = _scenarios()   # (names and geometry only: nothing here asks the oracle, which a session builds after collection)


def calls_of(s):
    """the dirt calls of a scenario, in order; none: a fresh context"""
    return history(s.hist, s.target, s.family)


def group(name):
    return [s for g, s in SCENARIOS if g == name]


def ids(scenarios):
    return [s.name for s in scenarios]


# ---- the conditions (tests/test_history_cpu.py) ----------------------------------------------------------------------------------

def pairs(s):
    """-> [(dirt picture, dirt is noise, dirt stream, target picture or stream, target stream, target is noise)] of a scenario:
    image i of every dirt call against image i of the target"""
    t = s.target
    if isinstance(t, EncTarget):
        pics, _ = encoder_pictures(t.W, t.H, t.Cn, t.content)
        rows = [(p, orc.encode(p)[0]) for p in pics]
    else:
        rows = [(r, r) for r in rows_of(t)]
    out = []
    for cl in calls_of(s):
        depth = DEPTH.get(cl.how, 8)
        for i, (what, stream) in enumerate(rows):
            out.append((dirt_picture(cl.W, cl.H, cl.Cn, cl.kind, depth, i), cl.kind == "noise", dirt_stream(cl.W, cl.H, cl.Cn, cl.kind, depth, i),
                        what, stream, getattr(t, "content", "") == "noise"))
    return out


def covers(cl, t):
    """Does dirt call cl size every slot of its family at least as the target call will?  Batch, samples and stream stride."""
    ok = cl.n >= t.n and cl.W * cl.H * cl.Cn >= t.W * t.H * t.Cn
    if isinstance(t, Target):
        ok = ok and cl.stride >= stride_of(rows_of(t))
    return ok
