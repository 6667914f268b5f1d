"""CPU: delta chains on the oracle (tests/chain.py) — exact round trips of runs of successor frames (full-range runs whose
residuals leave int16 among them), the fold's rule for windows that stay as they are, the conditions the clamp fixture of
tests/test_chain_gpu.py must meet at every link, dwtx_view_chain_check against sets of sample addresses, and the three entry
points declared, typed and exported."""
import inspect

import numpy as np
import pytest

import chain
import delta
import test_delta_cpu as DC


# ---- round trips -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", delta.RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", delta.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_chain_round_trip(wh, C, rng):
    (W, H), (lo, hi) = wh, rng
    n = 4
    fr = chain.frames(W, H, C, lo, hi, n)
    assert len(fr) == n + 1 and all(f.dtype == delta.dtype_of(lo, hi) and f.min() >= lo and f.max() <= hi for f in fr)
    assert all((fr[i] != fr[i + 1]).any() for i in range(n))
    junk = [np.full_like(fr[0], lo + 1 + i) for i in range(n)]
    windows, links = chain.decode(chain.streams(fr), fr[0], junk, W, H, C, lo, hi)
    for i in range(n):
        assert links[i] is windows[i] and windows[i].dtype == fr[0].dtype and (windows[i] == fr[i + 1]).all(), i


@pytest.mark.parametrize("sgn", [0, 1], ids=["uint16", "int16"])
@pytest.mark.parametrize("wh", delta.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_full_range_chain_round_trip(wh, sgn):
    W, H = wh
    n = 4
    fr = chain.full_range_frames(W, H, sgn, n)
    lo, hi = (-32768, 32767) if sgn else (0, 65535)
    for i in range(n):
        d = delta.residual(fr[i + 1], fr[i])
        assert d.min() < -32768 or d.max() > 32767, i
        assert delta.stream(fr[i + 1], fr[i])[1].planes[0] <= 16, i
    windows, _ = chain.decode(chain.streams(fr), fr[0], [np.zeros_like(fr[0])] * n, W, H, 1, lo, hi)
    assert all((w == f).all() for w, f in zip(windows, fr[1:]))


def test_a_window_that_stays_is_the_next_base():
    """An unreadable stream and one cut before its finest level keep what the caller left, and the next link adds its residual to
    THAT, not to the frame that was coded."""
    import levels
    import orc

    W, H, C, lo, hi = 132, 72, 1, 0, 255
    fr = chain.frames(W, H, C, lo, hi, 4)
    datas = chain.streams(fr)
    datas[1] = datas[1][:5]
    datas[2] = levels.late_prefix(datas[2], W, H, C, orc.geometry(W, H).levels - 2)
    left = [np.full_like(fr[0], 40 + 50 * i) for i in range(4)]
    windows, links = chain.decode(datas, fr[0], left, W, H, C, lo, hi)
    assert links[1] is None and links[2] is chain.UNTOUCHED
    assert (windows[0] == fr[1]).all() and windows[1] is left[1] and windows[2] is left[2]
    want = np.clip(left[2].astype(np.int64) + delta.residual(fr[4], fr[3]), lo, hi)
    assert (windows[3] == want).all() and (windows[3] != fr[4]).any()


# ---- the clamp fixture -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", delta.RANGES, ids=lambda r: "%d..%d" % r)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("wh", delta.SHAPES, ids=lambda wh: "%dx%d" % wh)
def test_clamp_fixture_meets_its_conditions_at_every_link(wh, C, rng):
    """At EVERY link, with the running decoded base: the finest level is reached and delta.clamps_are_at_work holds; from link 2
    on at least 20 % of the samples differ from what the true previous frame as base would give — which is what makes a kernel
    that reads a stale or a wrong base visible."""
    (W, H), (lo, hi) = wh, rng
    report = chain.clamp_fixture_report(W, H, C, lo, hi)
    assert len(report) == 4
    for i, (finest, work, shares, differ) in enumerate(report):
        print(wh, C, rng, "link", i, finest, work, shares, "differ %.3f" % differ)
    for i, (finest, work, shares, differ) in enumerate(report):
        assert finest and work, (i, shares)
        if i >= 2:
            assert differ >= 0.20, (i, differ)


# ---- dwtx_view_chain_check ---------------------------------------------------------------------------------------------------------

def _random_key(rng, W, H, Cn):
    """One window in any form a view takes: dense, pitched, stepped, planar."""
    kinds = ["dense", "pitched", "stepped"] + (["planar"] if Cn == 3 else [])
    kind = kinds[rng.integers(len(kinds))]
    if kind == "dense":
        return kind, DC._fields(W, H, Cn, 1, W * Cn, 0)
    if kind == "pitched":
        return kind, DC._fields(W, H, Cn, 1, W * Cn + int(rng.integers(1, 12)), 0)
    if kind == "stepped":
        step = Cn + int(rng.integers(1, 3))
        return kind, DC._fields(W, H, Cn, 1, W * step + int(rng.integers(0, 4)), 0, pixel_step=step)
    pitch = W + int(rng.integers(0, 4))
    return kind, DC._fields(W, H, Cn, 1, pitch, 0, channel_stride=H * pitch + int(rng.integers(0, 5)))


def test_chain_check_against_address_sets():
    """400 seeded pairs of a grid and a key at random distances: wherever the check accepts a decode, the key shares no byte with
    the destination; every encode is accepted; both answers occur often enough to mean something, for every kind of grid and key."""
    import dwt_amd

    rng = np.random.default_rng(12)
    W, H = 9, 8
    taken = refused = wrongly = 0
    seen = set()
    for _ in range(400):
        Cn = (1, 3)[int(rng.integers(2))]
        sb = (1, 2)[int(rng.integers(2))]
        n = int(rng.integers(3, 5))
        kind, f = DC._random_grid(rng, W, H, Cn, n)
        if rng.integers(4) == 0:   # a key of the windows' own form: one of them, moved
            kk, fk = "own", dict(f, n=1, cols=0, image_stride=0, band_stride=0)
        else:
            kk, fk = _random_key(rng, W, H, Cn)
        ptr = 1 << 24
        span = DC._span(f) * sb
        kspan = DC._span(fk) * sb
        d = int(rng.integers(-kspan - 64, span + 64)) * sb if rng.integers(4) else (span + 1024 * sb if rng.integers(2) else -kspan - 1024 * sb)
        kptr = ptr + d
        rc_e, _ = dwt_amd.view_chain_check(f, fk, ptr, kptr, sample_bytes=sb, dst=False)
        rc_d, text = dwt_amd.view_chain_check(f, fk, ptr, kptr, sample_bytes=sb, dst=True)
        assert rc_e == 0, (kind, kk, f, fk)
        A, K = DC._addresses(f, ptr, sb), DC._addresses(fk, kptr, sb)
        if rc_d == 0:
            taken += 1
            assert not (A & K), (kind, kk, f, fk, d)
        else:
            refused += 1
            wrongly += not (A & K)   # (sufficient, not necessary: a key between the windows' rows on another lattice is refused)
            assert rc_d == -3 and "meets the key" in text, text
        seen.add((kind, kk, rc_d == 0))
    print(taken, refused, wrongly, sorted(seen))
    assert taken >= 60 and refused >= 60
    for k in ("stack", "beside", "bands", "stepped", "nchw", "cnhw"):
        assert any(s[0] == k and s[2] for s in seen) and any(s[0] == k and not s[2] for s in seen), k
    for k in ("own", "dense", "pitched", "stepped", "planar"):
        assert any(s[1] == k and s[2] for s in seen) and any(s[1] == k and not s[2] for s in seen), k


def test_chain_check_named_layouts():
    import dwt_amd

    W, H, n = 16, 8, 3
    frame = H * W
    ptr = 1 << 24
    check = dwt_amd.view_chain_check
    stack = DC._fields(W, H, 1, n, W, frame)
    one = DC._fields(W, H, 1, 1, W, 0)
    # t[0] as key, t[1:] as destination: taken, with both sample sizes; so is a key in another allocation, and one behind the stack
    assert check(stack, one, ptr + frame, ptr, dst=True) == (0, "")
    assert check(stack, one, ptr + 2 * frame, ptr, sample_bytes=2, dst=True) == (0, "")
    assert check(stack, one, ptr, ptr + (1 << 20), dst=True) == (0, "")
    assert check(stack, one, ptr, ptr + n * frame, dst=True) == (0, "")
    # key == window 0, key == window 2, key one row down into a window: refused as decodes, taken as encodes
    for kptr, window in ((ptr, 0), (ptr + 2 * frame, 2), (ptr + W, 0), (ptr - W, 0)):
        rc, text = check(stack, one, ptr, kptr, dst=True)
        assert rc == -3 and "window %d of the destination meets the key" % window in text, text
        assert check(stack, one, ptr, kptr, dst=False) == (0, "")
    # windows with a pitch gap as wide as a row: a key of the same pitch inside the gap is taken, one column early it is not
    pitched = DC._fields(W, H, 1, n, 2 * W, H * 2 * W)
    gap_key = DC._fields(W, H, 1, 1, 2 * W, 0)
    assert check(pitched, gap_key, ptr, ptr + W, dst=True) == (0, "")
    assert check(pitched, gap_key, ptr, ptr + 2 * W, sample_bytes=2, dst=True) == (0, "")   # (addresses count bytes)
    assert check(pitched, gap_key, ptr + W, ptr, dst=True) == (0, "")            # (the windows in the key's gap)
    rc, text = check(pitched, gap_key, ptr, ptr + W - 1, dst=True)
    assert rc == -3 and "meets the key" in text, text
    rc, text = check(pitched, one, ptr, ptr + W, dst=True)                      # (a dense key there runs through the windows' rows)
    assert rc == -3 and "meets the key" in text, text
    # a planar key under an interleaved stack, and the other way round
    planar = DC._fields(W, H, 3, 1, W, 0, channel_stride=frame)
    inter = DC._fields(W, H, 3, n, 3 * W, 3 * frame)
    assert check(inter, planar, ptr + 3 * frame, ptr, dst=True) == (0, "")
    rc, text = check(inter, planar, ptr + 3 * frame, ptr + 1, dst=True)          # (its B plane's last row reaches into window 0)
    assert rc == -3 and "window 0 of the destination meets the key" in text, text
    nchw = DC._fields(W, H, 3, n, W, 3 * frame, channel_stride=frame)
    assert check(nchw, DC._fields(W, H, 3, 1, 3 * W, 0), ptr + 3 * frame, ptr, dst=True) == (0, "")
    # the key's cols, image_stride and band_stride are not looked at
    odd = dict(one, cols=7, image_stride=3, band_stride=5)
    assert check(stack, odd, ptr + frame, ptr, dst=True) == (0, "")
    # a NULL key, and mismatches, in either direction
    for dst in (False, True):
        for fk, kptr in ((None, 0), (one, 0)):
            rc, text = check(stack, fk, ptr, kptr, dst=dst)
            assert rc == -3 and "no key" in text, text
        rc, text = check(inter, one, ptr, ptr + (1 << 20), dst=dst)
        assert rc == -3 and "3 channels, its key 1" in text, text
        rc, text = check(stack, one, ptr, ptr + (1 << 20), sample_bytes=2, key_sample_bytes=1, dst=dst)
        assert rc == -3 and "2-byte samples, its key 1-byte" in text, text
        rc, text = check(stack, one, ptr, ptr + (1 << 20), sample_bytes=1, signed=True, dst=dst)
        assert rc == -3 and "int16_t" in text, text
        rc, text = check(stack, one, ptr, ptr + (1 << 20), sample_bytes=2, minval=-5, dst=dst)
        assert rc == -3 and "without sgn" in text, text
    # a signed range outside the rule (decodes read it), and 8-bit samples with another maxval
    rc, text = check(stack, one, ptr, ptr + (1 << 20), sample_bytes=2, signed=True, minval=100, maxval=50, dst=True)
    assert rc == -3 and "minval < maxval" in text, text
    assert check(stack, one, ptr, ptr + (1 << 20), sample_bytes=2, signed=True, minval=-1024, maxval=3071, dst=True) == (0, "")
    rc, text = check(stack, one, ptr, ptr + (1 << 20), sample_bytes=1, maxval=100, dst=True)
    assert rc == -3 and "maxval 100" in text, text
    # the destination's own rules still hold: windows that overlap one another
    rc, text = check(DC._fields(W, H, 1, n, W, frame - W), one, ptr, ptr + (1 << 20), dst=True)
    assert rc == -3 and "windows overlap" in text, text


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------

def test_chain_entry_points_are_declared_typed_and_exported():
    from dwt_amd import _lib
    import dwt_amd
    import test_abi

    lib = _lib.load()
    declared = test_abi.declared_symbols()
    for name in ("dwtx_encode_view_chain", "dwtx_decode_view_chain", "dwtx_view_chain_check"):
        assert name in declared, f"{name} is not declared in include/dwtx.h"
        assert name in _lib.SYMBOLS, f"{name} is not typed in dwt_amd/_lib.py"
        assert hasattr(lib, name), f"{name} is not exported by libdwtx.so"
    for fn in (dwt_amd.Context.encode_view_chain, dwt_amd.Context.decode_view_chain):
        assert "key" in inspect.signature(fn).parameters, fn
    assert callable(dwt_amd.view_chain_check)
