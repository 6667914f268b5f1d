"""CPU: delta views on the oracle (tests/delta.py) — the decoder's clamps by hand, exact round trips (full-range pictures
whose residuals leave int16 among them), the plane bound of a residual's doubled range, the condition the clamp fixtures of
tests/test_delta_gpu.py must meet, dwtx_view_delta_check against sets of sample addresses, and the three entry points
declared, typed and exported."""
import inspect

import numpy as np
import pytest

import deep
import delta
import orc
import test_deep_cpu as D


# ---- by hand ---------------------------------------------------------------------------------------------------------------------

def test_gray_delta_by_hand():
    """[0, 255], R = 255, a 2 x 3 picture.  The residual's clamp at either end (-300 -> -255, 300 -> 255), then the final clamp at
    either end (250 + 10, 5 - 10), and two samples that no clamp touches."""
    img = np.array([[[-300], [300], [10]], [[-10], [100], [-100]]])
    B = np.array([[[200], [50], [250]], [[5], [100], [100]]], dtype=np.uint8)
    got = delta.delta_pixels(img, B, 1, 0, 255)
    assert got.dtype == np.uint8 and got.tolist() == [[[0], [255], [255]], [[0], [200], [0]]]
    # the same residual in a signed range of the same width lands minval lower
    got = delta.delta_pixels(img, (B.astype(np.int16) - 100), 1, -100, 155)
    assert got.dtype == np.int16 and got.tolist() == [[[-100], [155], [155]], [[-100], [100], [-100]]]
    # R = 65535: nothing of a full-range residual is clamped before the sum
    img = np.array([[[-65535], [65535], [70000]]])
    B = np.array([[[65535], [0], [3]]], dtype=np.uint16)
    assert delta.delta_pixels(img, B, 1, 0, 65535).tolist() == [[[0], [65535], [65535]]]


def test_rgb_delta_by_hand():
    """[0, 255], R = 255, a 2 x 3 picture of (Y, Co, Cg); every clamp once and with both signs.
    (300, 0, 0): Y -> 255, d = (255, 255, 255).  (-300, 0, 0): d = (-255, -255, -255).
    (0, 600, 0): Co -> 510: T = 0, G = 0, B = 0 - 255 = -255, R = -255 + 510 = 255.  (0, -600, 0): Co -> -510: B = 0 + 255, R = 255 -
    510 = -255.  (0, 0, 600): Cg -> 510: T = -255, G = 510 - 255 = 255, B = R = -255.  (0, 0, -600): Cg -> -510: T = 255, G = -510 +
    255 = -255, B = R = 255.  The bases are chosen so that each sum is clamped at an end or left alone."""
    img = np.array([[[300, 0, 0], [-300, 0, 0], [0, 600, 0]], [[0, -600, 0], [0, 0, 600], [0, 0, -600]]])
    B = np.array([[[0, 10, 250], [255, 100, 0], [10, 20, 255]], [[255, 20, 0], [255, 0, 255], [0, 255, 0]]], dtype=np.uint8)
    want = [[[255, 255, 255], [0, 0, 0], [255, 20, 0]], [[0, 20, 255], [0, 255, 0], [255, 0, 255]]]
    assert delta.delta_pixels(img, B, 3, 0, 255).tolist() == want
    # the residual's own clamp: (255, 510, 0) is inside every input clamp and gives R = 510 -> 255
    assert delta.clamp_residual(np.array([[[255, 510, 0]]]), 3, 255).tolist() == [[[255, 255, 0]]]
    # a residual no clamp touches comes back as S
    S = np.array([[[7, 200, 31], [0, 255, 128]]], dtype=np.uint8)
    Bs = np.array([[[250, 3, 30], [255, 0, 127]]], dtype=np.uint8)
    assert (delta.delta_pixels(deep.rgb2ycocg(delta.residual(S, Bs)), Bs, 3, 0, 255) == S).all()


# ---- round trips -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", delta.RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", delta.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_delta_round_trip(wh, C, rng):
    (W, H), (lo, hi) = wh, rng
    S, B = delta.successor(W, H, C, lo, hi, 1)
    assert S.dtype == B.dtype == delta.dtype_of(lo, hi) and S.min() >= lo and S.max() <= hi and (S != B).any()
    data, st = delta.stream(S, B)
    assert max(list(st.planes)[:C]) <= 16
    own = deep.deep_encode(S)[0]
    print(W, H, C, rng, "own", len(own), "delta", len(data))
    assert len(data) < len(own)
    back = delta.delta_decode(data, B, W, H, C, lo, hi)
    assert back.dtype == S.dtype and (back == S).all()


@pytest.mark.parametrize("sgn", [0, 1], ids=["uint16", "int16"])
@pytest.mark.parametrize("wh", delta.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_full_range_residuals_leave_int16_and_round_trip(wh, sgn):
    W, H = wh
    S, B = delta.full_range_pair(W, H, sgn)
    d = delta.residual(S, B)
    assert d.min() < -32768 and d.max() > 32767
    data, st = delta.stream(S, B)
    assert st.planes[0] <= 16
    lo, hi = (-32768, 32767) if sgn else (0, 65535)
    assert (delta.delta_decode(data, B, W, H, 1, lo, hi) == S).all()


def test_the_noise_pair_is_refused():
    for sgn in (0, 1):
        assert delta.stream(*delta.noise_pair(132, 72, sgn))[1].planes[0] > 16


def test_unreadable_and_reduced_streams():
    import levels

    W, H = 263, 135
    S, B = delta.clamp_pair(W, H, 1, 0, 255)
    data = delta.stream(S, B)[0]
    assert delta.delta_decode(data[:5], B, W, H, 1, 0, 255) is None
    T = orc.geometry(W, H).levels
    assert delta.delta_decode(levels.late_prefix(data, W, H, 1, T - 2), B, W, H, 1, 0, 255) is delta.UNTOUCHED


# ---- the plane bound ---------------------------------------------------------------------------------------------------------------

_gain = {}


def _detail_top(D_):
    H, W, C = D_.shape
    g = orc.geometry(W, H)
    pyr = orc.forward(deep.rgb2ycocg(D_) if C == 3 else D_.astype(np.int32))
    pyr[:g.heights[0], :g.widths[0]] = 0
    return int(np.abs(pyr).max())


def _worst_residuals(g, R):
    """deep.Gain's worst pictures as residuals of two pictures in [0, R]: S the worst picture and B = R - S, so that D = 2S - R
    has +-R where S has R and 0 — gray by the signed response (crows: a residual is a signed input), and as the unsigned
    winner; RGB with Co = +-2R."""
    ay, ax = g.crows
    Sg = ((np.outer(ay, ax) > 0) * R).astype(np.int64)[..., None]
    Su = g.worst_gray(R).astype(np.int64)
    Sc = g.worst_rgb(R).astype(np.int64)
    Sc[..., 1] = np.where(Sc[..., 0] > 0, 0, R)   # (G against R and B: Cg = +-2R as well, where worst_rgb leaves it near 0)
    return [("gray, signed response", 2 * Sg - R), ("gray, unsigned winner", 2 * Su - R), ("rgb, Co", 2 * g.worst_rgb(R).astype(np.int64) - R),
            ("rgb, Co and Cg", 2 * Sc - R)]


@pytest.mark.parametrize("wh", D.GEOMETRIES, ids=lambda wh: "%dx%d" % wh)
def test_residuals_of_these_ranges_never_need_more_than_16_planes(wh):
    """A residual lies in [-R, R], a range of 2R: by DESIGN.md sections 4.8 and 4.20 (gray ranges up to 8191, RGB up to 4095) gray
    pictures with R <= 4095 and RGB ones with R <= 2047 cannot need more than 16 planes — all 8-bit pictures among them."""
    g = _gain.setdefault(wh, deep.Gain(*wh))
    for R_gray, R_rgb in ((4095, 2047), (255, 255)):
        for name, D_ in _worst_residuals(g, R_gray)[:2] + _worst_residuals(g, R_rgb)[2:]:
            assert np.abs(D_).max() <= (R_gray if D_.shape[2] == 1 else R_rgb)
            top = _detail_top(D_)
            print(wh, name, R_gray if D_.shape[2] == 1 else R_rgb, top)
            assert top < 1 << 16, name


# ---- the clamp fixtures ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", delta.RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", delta.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_clamp_fixtures_meet_their_condition(wh, C, rng):
    (W, H), (lo, hi) = wh, rng
    for cut in delta.CUTS:
        data, B = delta.cut_fixture(W, H, C, lo, hi, cut)
        r = deep.decoded(data, W, H, C)
        assert r is not None
        print(wh, C, rng, cut, "level", r[0], delta.clamp_shares(r[3], B, C, lo, hi))
        assert r[0] == orc.geometry(W, H).levels - 1
        assert delta.clamps_are_at_work(r[3], B, W, H, C, lo, hi)
        S = delta.clamp_pair(W, H, C, lo, hi)[0]
        got = delta.delta_decode(data, B, W, H, C, lo, hi)
        assert got.shape == S.shape and (got != S).any()   # an approximation: the stream lost planes


# ---- dwtx_view_delta_check -------------------------------------------------------------------------------------------------------

def _fields(W, H, Cn, n, row_pitch, image_stride, cols=0, band_stride=0, channel_stride=0, pixel_step=0):
    return dict(W=W, H=H, channels=Cn, n=n, cols=cols, row_pitch=row_pitch, image_stride=image_stride, band_stride=band_stride,
                channel_stride=channel_stride, pixel_step=pixel_step)


def _addresses(f, ptr, sb):
    """Every byte address of every sample of a grid view."""
    out = set()
    Cn = f["channels"]
    step = 1 if f["channel_stride"] else (f["pixel_step"] or Cn)
    cstep = f["channel_stride"] or 1
    cols = f["cols"] if f["cols"] and f["cols"] < f["n"] else 0
    for i in range(f["n"]):
        w0 = i * f["image_stride"] if not cols else (i // cols) * f["band_stride"] + (i % cols) * f["image_stride"]
        for c in range(Cn):
            for y in range(f["H"]):
                base = ptr + sb * (w0 + c * cstep + y * f["row_pitch"])
                out.update(base + sb * step * x + b for x in range(f["W"]) for b in range(sb))
    return out


def _random_grid(rng, W, H, Cn, n):
    """A grid view of n windows that are disjoint among themselves: a stack, windows side by side, bands, planar in both forms,
    or stepped."""
    kinds = ["stack", "beside", "bands", "stepped"] + (["nchw", "cnhw"] if Cn == 3 else [])
    kind = kinds[rng.integers(len(kinds))]
    pad = int(rng.integers(0, 4))
    if kind == "stack":
        pitch = W * Cn + pad
        return kind, _fields(W, H, Cn, n, pitch, H * pitch + int(rng.integers(0, 9)))
    if kind == "beside":
        img = W * Cn + pad
        return kind, _fields(W, H, Cn, n, n * img + int(rng.integers(0, 5)), img)
    if kind == "bands":
        img = W * Cn + pad
        pitch = 2 * img + int(rng.integers(0, 5))
        return kind, _fields(W, H, Cn, n, pitch, img, cols=2, band_stride=H * pitch + int(rng.integers(0, 9)))
    if kind == "stepped":
        step = Cn + int(rng.integers(1, 3))
        pitch = W * step + pad
        return kind, _fields(W, H, Cn, n, pitch, H * pitch + pad, pixel_step=step)
    if kind == "nchw":
        cs = H * (W + pad) + int(rng.integers(0, 5))
        return kind, _fields(W, H, Cn, n, W + pad, 3 * cs + int(rng.integers(0, 5)), channel_stride=cs)
    pitch = W + pad                                  # cnhw: the three planes of the whole view apart
    img = H * pitch + int(rng.integers(0, 5))
    return kind, _fields(W, H, Cn, n, pitch, img, channel_stride=n * img + int(rng.integers(0, 9)))


def _span(f):
    return max(_addresses(f, 0, 1)) + 1


def test_delta_check_against_address_sets():
    """Seeded pairs of grids at random distances: wherever the check accepts a decode, the two views are the same view or share no
    byte; every encode is accepted; and both answers occur often enough to mean something."""
    import dwt_amd

    rng = np.random.default_rng(11)
    W, H = 9, 8
    taken = refused = 0
    seen = set()
    for _ in range(400):
        Cn = (1, 3)[int(rng.integers(2))]
        sb = (1, 2)[int(rng.integers(2))]
        n = int(rng.integers(3, 5))
        kind, f = _random_grid(rng, W, H, Cn, n)
        same = rng.integers(5) == 0
        kb, fb = (kind, dict(f)) if same or rng.integers(2) else _random_grid(rng, W, H, Cn, n)
        ptr = 1 << 24
        span = _span(f) * sb
        d = 0 if same else int(rng.integers(-span - 64, span + 64)) * sb if rng.integers(3) else span + 1024 * sb
        bptr = ptr + d
        rc_e, _ = dwt_amd.view_delta_check(f, fb, ptr, bptr, sample_bytes=sb, dst=False)
        rc_d, text = dwt_amd.view_delta_check(f, fb, ptr, bptr, sample_bytes=sb, dst=True)
        assert dwt_amd.view_delta_check(f, f, ptr, ptr, sample_bytes=sb, dst=True) == (0, ""), (kind, f)   # (in place)
        assert rc_e == 0, (kind, kb, f, fb)
        A, Bs = _addresses(f, ptr, sb), _addresses(fb, bptr, sb)
        identical = f == fb and ptr == bptr
        if rc_d == 0:
            taken += 1
            assert identical or not (A & Bs), (kind, kb, f, fb, d)
        else:
            refused += 1
            assert "meets window" in text, text
            assert not identical
        seen.add((kind, kb, rc_d == 0))
    print(taken, refused, sorted(seen))
    assert taken >= 60 and refused >= 60
    for k in ("stack", "beside", "bands", "stepped", "nchw", "cnhw"):
        assert any(s[0] == k and s[2] for s in seen) and any(s[0] == k and not s[2] for s in seen), k


def test_delta_check_named_layouts():
    import dwt_amd

    W, H, n = 16, 8, 3
    frame = H * W
    ptr = 1 << 24
    stack = _fields(W, H, 1, n, W, frame)
    check = dwt_amd.view_delta_check
    # taken: another tensor, even / odd frames of one stack, in place
    assert check(stack, stack, ptr, ptr + (1 << 20), dst=True) == (0, "")
    evens = _fields(W, H, 1, n, W, 2 * frame)
    assert check(evens, evens, ptr + frame, ptr, dst=True) == (0, "")
    assert check(evens, evens, ptr + 2 * frame, ptr, sample_bytes=2, dst=True) == (0, "")
    assert check(stack, stack, ptr, ptr, dst=True) == (0, "")
    planar = _fields(W, H, 3, n, W, 3 * frame, channel_stride=frame)
    inter = _fields(W, H, 3, n, 3 * W, 3 * frame)
    assert check(planar, inter, ptr, ptr + (1 << 20), dst=True) == (0, "")
    # refused as decodes, taken as encodes: t[1:] on t[:-1], a base one row down
    for bptr in (ptr - frame, ptr + W):
        rc, text = check(stack, stack, ptr, bptr, dst=True)
        assert rc == -3 and "meets window" in text and "chain" in text, text
        assert check(stack, stack, ptr, bptr, dst=False) == (0, "")
    # mismatches, in either direction
    for dst in (False, True):
        rc, text = check(inter, stack, ptr, ptr + (1 << 20), dst=dst)
        assert rc == -3 and "3 channels, its base 1" in text, text
        rc, text = check(stack, stack, ptr, ptr + (1 << 20), sample_bytes=2, base_sample_bytes=1, dst=dst)
        assert rc == -3 and "2-byte samples, its base 1-byte" in text, text
        rc, text = check(stack, stack, ptr, ptr + (1 << 20), sample_bytes=1, signed=True, dst=dst)
        assert rc == -3 and "int16_t" in text, text
        rc, text = check(stack, stack, ptr, ptr + (1 << 20), sample_bytes=2, minval=-5, dst=dst)
        assert rc == -3 and "without sgn" in text, text
    # a signed range outside the rule (decodes read it), and 8-bit samples with another maxval
    rc, text = check(stack, stack, ptr, ptr + (1 << 20), sample_bytes=2, signed=True, minval=100, maxval=50, dst=True)
    assert rc == -3 and "minval < maxval" in text, text
    assert check(stack, stack, ptr, ptr + (1 << 20), sample_bytes=2, signed=True, minval=-1024, maxval=3071, dst=True) == (0, "")
    rc, text = check(stack, stack, ptr, ptr + (1 << 20), sample_bytes=1, maxval=100, dst=True)
    assert rc == -3 and "maxval 100" in text, text


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

def test_delta_entry_points_are_declared_typed_and_exported():
    from dwt_amd import _lib, tiles
    import dwt_amd
    import test_abi

    lib = _lib.load()
    declared = test_abi.declared_symbols()
    for name in ("dwtx_encode_view_delta", "dwtx_decode_view_delta", "dwtx_view_delta_check"):
        assert name in declared, f"{name} is not declared in include/dwtx.h"
        assert name in _lib.SYMBOLS, f"{name} is not typed in dwt_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libdwtx.so"
    for fn in (dwt_amd.Context.encode_view, dwt_amd.Context.decode_view, tiles.encode_frame, tiles.decode_frame):
        assert "base" in inspect.signature(fn).parameters, fn
    assert callable(dwt_amd.view_delta_check)
