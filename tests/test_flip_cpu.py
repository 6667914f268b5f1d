"""CPU: flips in views (dwtx_view_flip_plan, include/dwtx.h) — the table a flipped call walks its windows with, and what
the two *_view_flip calls refuse.  Host arithmetic only: pointers are plain integers and are never dereferenced.

The helpers of tests/flip.py — what tests/test_flip_gpu.py builds its expectations with — are held against hand-written
cases first.  Then the plan is held against brute force: a flat buffer of running numbers, each window's positive view of it
(numpy's as_strided, as tests/test_views_gpu.py builds them), and the view the plan's origin and SIGNED strides give, which
must be np.flip of the former for every window.  The layouts are the seeded lists of tests/test_list_cpu.py and the stack,
band and grid layouts of the GPU tests, with interleaved, planar and stepped rows, under random per-window flags."""
import random

import numpy as np
import pytest

import dwt_amd
import flip
import test_list_cpu as LC
import test_planar_gpu as P
import test_step_gpu as S
import test_views_gpu as V

ERR_ARG = -3
BASE = LC.BASE


# ---- the helpers ------------------------------------------------------------------------------------------------------------

A23 = np.array([[1, 2, 3],
                [4, 5, 6]])
A44 = np.arange(16).reshape(4, 4)


def test_in_memory_by_hand():
    want23 = {0: [[1, 2, 3], [4, 5, 6]], 1: [[3, 2, 1], [6, 5, 4]], 2: [[4, 5, 6], [1, 2, 3]], 3: [[6, 5, 4], [3, 2, 1]]}
    want44 = {0: [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]],
              1: [[3, 2, 1, 0], [7, 6, 5, 4], [11, 10, 9, 8], [15, 14, 13, 12]],
              2: [[12, 13, 14, 15], [8, 9, 10, 11], [4, 5, 6, 7], [0, 1, 2, 3]],
              3: [[15, 14, 13, 12], [11, 10, 9, 8], [7, 6, 5, 4], [3, 2, 1, 0]]}
    for f in flip.FLAGS:
        assert flip.in_memory(A23, f).tolist() == want23[f], f
        assert flip.in_memory(A44, f).tolist() == want44[f], f
    # the definition itself: memory (x, y) holds picture (u, v)
    for f in flip.FLAGS:
        m = flip.in_memory(A44, f)
        for y in range(4):
            for x in range(4):
                u, v = (3 - x if f & 1 else x), (3 - y if f & 2 else y)
                assert m[y, x] == A44[v, u]
    # channels ride along: [H, W, C]
    rgb = np.arange(2 * 3 * 3).reshape(2, 3, 3)
    assert flip.in_memory(rgb, 1)[0, 0].tolist() == rgb[0, 2].tolist() and flip.in_memory(rgb, 2)[0, 0].tolist() == rgb[1, 0].tolist()


def test_in_memory_is_an_involution():
    rng = np.random.default_rng(5)
    for shape in ((2, 3), (4, 4), (5, 7, 3), (1, 9, 1)):
        a = rng.integers(0, 255, shape)
        for f in flip.FLAGS:
            assert (flip.in_memory(flip.in_memory(a, f), f) == a).all()
            assert (flip.in_memory(a, f) == np.flip(a, [ax for ax, bit in ((1, 1), (0, 2)) if f & bit])).all() if f else True


def test_place_by_hand():
    """a 1x2 picture in a 2x3 window, a 2x2 one in a 4x4 window: the corner where pixel (0, 0) lies"""
    part = np.array([[7, 8]])
    want23 = {0: [[7, 8, 0], [0, 0, 0]], 1: [[0, 8, 7], [0, 0, 0]], 2: [[0, 0, 0], [7, 8, 0]], 3: [[0, 0, 0], [0, 8, 7]]}
    part44 = np.array([[1, 2], [3, 4]])
    want44 = {0: [[1, 2, 0, 0], [3, 4, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]],
              1: [[0, 0, 2, 1], [0, 0, 4, 3], [0, 0, 0, 0], [0, 0, 0, 0]],
              2: [[0, 0, 0, 0], [0, 0, 0, 0], [3, 4, 0, 0], [1, 2, 0, 0]],
              3: [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 4, 3], [0, 0, 2, 1]]}
    for f in flip.FLAGS:
        w = np.zeros((2, 3), dtype=int)
        flip.place(w, part, f)
        assert w.tolist() == want23[f], f
        w = np.zeros((4, 4), dtype=int)
        flip.place(w, part44, f)
        assert w.tolist() == want44[f], f
        full = np.zeros((4, 4), dtype=int)
        flip.place(full, A44, f)   # a picture that fills its window is in_memory
        assert (full == flip.in_memory(A44, f)).all()


# ---- the plan against brute force ------------------------------------------------------------------------------------------------

def plan_of_layout(L, flags, dst, sample_bytes=1):
    """dwtx_view_flip_plan for a Layout of the GPU tests (a grid: no pointers)"""
    H, W, Cn = L.shape[-3:]
    sh, sw, sc = L.strides[-3:]
    planar = Cn == 3 and sw == 1 and sc > 1
    step = 0 if planar or sw == Cn else sw
    if len(L.shape) == 4:
        cols, image_stride, band_stride = 0, L.strides[0], 0
    else:
        cols, image_stride, band_stride = L.shape[1], L.strides[1], L.strides[0]
    return dwt_amd.view_flip_plan(W, H, L.n, 0, None, channels=Cn, row_pitch=sh, image_stride=image_stride, cols=cols, band_stride=band_stride,
                                  channel_stride=sc if planar else 0, pixel_step=step, sample_bytes=sample_bytes, dst=dst, flips=flags)


GRIDS = [
    ("stack", lambda W, H: V.stack(W, H, 3, n=5)), ("stack-gray", lambda W, H: V.stack(W, H, 1, n=5)),
    ("band", lambda W, H: V.band(W, H, 3)), ("grid", lambda W, H: V.grid(W, H, 3)), ("grid-gray", lambda W, H: V.grid(W, H, 1, rows=2, cols=3)),
    ("nchw", lambda W, H: P.nchw(W, H, n=5)), ("chw_grid", lambda W, H: P.chw_grid(W, H)), ("cnhw", lambda W, H: P.cnhw(W, H)),
    ("rgba-stack", lambda W, H: S.sstack(W, H, 3, 4, n=5)), ("rgba-band", lambda W, H: S.sband(W, H, 3, 4)), ("rgba-grid", lambda W, H: S.sgrid(W, H, 3, 4)),
    ("mosaic-grid", lambda W, H: S.sgrid(W, H, 1, 2, rows=2, cols=2)),
]


@pytest.mark.parametrize("name,make", GRIDS, ids=[g[0] for g in GRIDS])
def test_the_plan_of_a_grid_walks_the_flipped_windows(name, make):
    rng = random.Random(len(name) * 131 + 7)
    for W, H in ((12, 10), (9, 8), (8, 13)):
        L = make(W, H)
        Cn = L.shape[-1]
        cs = L.strides[-1]
        buf = np.arange(L.samples, dtype=np.int64)
        wins = L.np_windows(buf)
        for flags in ([rng.randrange(4) for _ in range(L.n)], flip.MIXED[:L.n] + [0] * max(0, L.n - 5), [3] * L.n):
            for dst in (True, False):
                rc, text, origin, pitch, step = plan_of_layout(L, flags, dst)
                assert (rc, text) == (0, ""), (name, text)
                for i, f in enumerate(flags):
                    got = flip.walked(buf, L.off + origin[i], pitch[i], step[i], cs, H, W, Cn)
                    assert (got == flip.in_memory(wins[i], f)).all(), (name, i, f)
                    assert (got == np.flip(wins[i], [ax for ax, bit in ((1, 1), (0, 2)) if f & bit])).all() if f else (got == wins[i]).all()
                    assert abs(pitch[i]) == L.strides[-3] and (pitch[i] < 0) == bool(f & 2)
                    assert abs(step[i]) == L.strides[-2] and (step[i] < 0) == bool(f & 1)
        # one mask for all windows is the list of n of it
        for f in flip.FLAGS:
            assert dwt_amd.view_flip_plan(W, H, L.n, f, None, **_grid_kw(L)) == plan_of_layout(L, [f] * L.n, True)


def _grid_kw(L):
    H, W, Cn = L.shape[-3:]
    sh, sw, sc = L.strides[-3:]
    planar = Cn == 3 and sw == 1 and sc > 1
    four = len(L.shape) == 4
    return dict(channels=Cn, row_pitch=sh, image_stride=L.strides[0] if four else L.strides[1], cols=0 if four else L.shape[1],
                band_stride=0 if four else L.strides[0], channel_stride=sc if planar else 0, pixel_step=0 if planar or sw == Cn else sw)


def test_the_plan_of_the_seeded_lists_walks_the_flipped_windows():
    """the generator of tests/test_list_cpu.py: gray, RGB, stepped and planar units on a pitch lattice, half of them nudged.
    An encode takes every one of them; a decode those dwtx_view_list_check takes, with the same text where it does not."""
    rng = random.Random(20261)
    took = refused = 0
    for k in range(1200):
        starts, W, H, view = LC.random_list(rng, k)
        n, Cn = len(starts), view["channels"]
        cs = view["channel_stride"] or 1
        pstep = 1 if view["channel_stride"] else (view["pixel_step"] or Cn)
        flags = [rng.randrange(4) for _ in range(n)]
        lowest = min(starts)
        samples = max(starts) + 2 * cs + H * view["row_pitch"] + W * pstep + 8
        buf = np.arange(samples, dtype=np.int64)
        sample_bytes = (1, 2, 4)[k % 3]
        ptrs = [BASE + s * sample_bytes for s in starts]
        rc, text, origin, pitch, step = dwt_amd.view_flip_plan(W, H, n, 0, ptrs, sample_bytes=sample_bytes, dst=False, flips=flags, **view)
        assert (rc, text) == (0, ""), (k, text)
        for i, f in enumerate(flags):
            win = np.lib.stride_tricks.as_strided(buf[starts[i]:], (H, W, Cn), (view["row_pitch"] * 8, pstep * 8, cs * 8))
            got = flip.walked(buf, lowest + origin[i], pitch[i], step[i], cs, H, W, Cn)
            assert (got == flip.in_memory(win, f)).all(), (k, i, f)
        as_dst = dwt_amd.view_flip_plan(W, H, n, 0, ptrs, sample_bytes=sample_bytes, dst=True, flips=flags, **view)
        check = dwt_amd.view_list_check(ptrs, W, H, sample_bytes=sample_bytes, dst=True, **view)
        assert as_dst[:2] == check, k   # a flip does not change which samples a window covers
        if check[0] == 0:
            assert as_dst[2:] == (origin, pitch, step)
            took += 1
        else:
            refused += 1
    assert took >= 60 and refused >= 60, (took, refused)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

FAR = [BASE + i * 4096 for i in range(5)]


def refused(*args, **kw):
    rc, text, origin, pitch, step = dwt_amd.view_flip_plan(*args, **kw)
    assert rc == ERR_ARG and text.strip() and origin == pitch == step == [], (rc, text)
    return text


def test_bad_flags_are_refused_with_a_text():
    assert dwt_amd.view_flip_plan(8, 8, 5, 3, FAR)[0] == 0 and dwt_amd.view_flip_plan(8, 8, 5, 0, FAR, flips=flip.MIXED)[0] == 0
    for dst in (True, False):
        assert "4" in refused(8, 8, 5, 4, FAR, dst=dst)
        assert "-1" in refused(8, 8, 5, -1, FAR, dst=dst)
        text = refused(8, 8, 5, 0, FAR, flips=[0, 1, 4, 3, 1], dst=dst)
        assert "4" in text and "window 2" in text
        assert "255" in refused(8, 8, 5, 0, FAR, flips=[0, 1, 2, 3, 255], dst=dst)
        # a grid, too
        assert "4" in refused(8, 8, 5, 4, None, dst=dst)
        assert "window 0" in refused(8, 8, 5, 0, None, flips=[7, 0, 0, 0, 0], dst=dst)


def test_flags_for_all_together_with_flags_per_window_are_refused():
    for f in (1, 2, 3):
        text = refused(8, 8, 5, f, FAR, flips=flip.MIXED)
        assert "host_flips" in text
        refused(8, 8, 5, f, None, flips=[0] * 5)   # (zeros are flags per window all the same)


@pytest.mark.parametrize("name,ptrs,view,always", LC.layouts_refused(), ids=[l[0] for l in LC.layouts_refused()])
def test_what_the_list_check_refuses_is_refused_with_its_text(name, ptrs, view, always):
    for dst in (True, False):
        for flags in ([3] * len(ptrs), [0] * len(ptrs)):
            got = dwt_amd.view_flip_plan(LC.W, LC.H, len(ptrs), 0, ptrs, dst=dst, flips=flags, **view)
            want = dwt_amd.view_list_check(ptrs, LC.W, LC.H, dst=dst, **view)
            assert got[:2] == want, (name, dst)
            assert (got[0] == ERR_ARG and got[1].strip()) if dst or always else got[0] == 0, name


def test_counts_and_views_are_refused_as_the_list_check_refuses_them():
    far = [BASE + i * 4096 for i in range(8)]
    cases = [
        ("no windows", [], dict()),
        ("a pitch below the row", far, dict(channels=3, row_pitch=23)),
        ("two channels", far, dict(channels=2, row_pitch=16)),
        ("a step below the channels", far, dict(channels=3, pixel_step=2, row_pitch=64)),
        ("a maxval of 0 for a destination", far, dict(sample_bytes=2, maxval=0)),
    ]
    for what, ptrs, view in cases:
        got = dwt_amd.view_flip_plan(8, 8, len(ptrs), 3, ptrs, dst=True, **view)
        assert got[0] == ERR_ARG and got[1].strip(), what
        if ptrs:
            assert got[:2] == dwt_amd.view_list_check(ptrs, 8, 8, dst=True, **view), what
    assert refused(0, 8, 8, 1, far, row_pitch=8)
    many = [BASE + i * 64 for i in range(21846)]
    for dst, channels in ((True, 1), (False, 3)):
        assert dwt_amd.view_flip_plan(8, 8, 21845, 2, many[:21845], dst=dst, channels=channels)[0] == 0
        text = refused(8, 8, 21846, 2, many, dst=dst, channels=channels)
        assert "21846" in text or "65538" in text
        # the grid spelled out takes what the list takes
        assert dwt_amd.view_flip_plan(8, 8, 21845, 2, None, dst=dst, channels=channels)[0] == 0
        text = refused(8, 8, 21846, 2, None, dst=dst, channels=channels)
        assert "21846" in text or "65538" in text


def test_a_grid_that_overlaps_is_refused_as_the_grid_calls_refuse_it():
    ok = dwt_amd.view_flip_plan(12, 10, 4, 3, None, channels=3, row_pitch=36, image_stride=360)
    assert ok[0] == 0 and ok[2] == [9 * 36 + 11 * 3 + i * 360 for i in range(4)] and ok[3] == [-36] * 4 and ok[4] == [-3] * 4
    text = refused(12, 10, 4, 3, None, channels=3, row_pitch=36, image_stride=359)
    assert "overlap" in text
    assert dwt_amd.view_flip_plan(12, 10, 4, 3, None, channels=3, row_pitch=36, image_stride=359, dst=False)[0] == 0   # (an encode may read them)


# ---- the keyword of the package ----------------------------------------------------------------------------------------------

def test_the_flip_keyword():
    vf = dwt_amd.view_flips
    for nothing in (None, 0, "", [0, 0, 0], [None, 0, ""], np.zeros(3, dtype=np.int64)):
        assert vf(nothing, 3) is None
    assert vf("x", 3) == (1, None) and vf("y", 3) == (2, None) and vf("xy", 3) == (3, None) and vf(3, 3) == (3, None) and vf(np.int64(2), 3) == (2, None)
    f, arr = vf([0, "x", 2, "xy", 1], 5)
    assert f == 0 and list(arr) == flip.MIXED
    f, arr = vf(np.array([1, 0, 1]), 3)
    assert f == 0 and list(arr) == [1, 0, 1]
    for bad in (4, -1, "z", "xx", True, 1.0, [0, 4, 0], [0, "q", 0], [0, 1], [0, 1, 2, 3], [[1], [0], [0]]):
        with pytest.raises(ValueError):
            vf(bad, 3)


def test_the_tiles_of_a_flipped_frame_are_listed_in_picture_order():
    import torch

    from dwt_amd import tiles

    FW, FH, tile = 150, 100, 64
    mem = torch.arange(FH * FW * 3, dtype=torch.int32).reshape(FH, FW, 3)
    for f in (1, 2, 3):
        upright = flip.in_memory(mem.numpy(), f)
        groups = dwt_amd.tile_groups(FW, FH, tile)
        assert len(groups) == 4
        seen = np.zeros((FH, FW), dtype=int)
        for g in groups:
            wins = tiles.group_windows(mem, g, f)
            assert len(wins) == g.rows * g.cols
            for i, w in enumerate(wins):
                y, x = g.y0 + (i // g.cols) * g.H, g.x0 + (i % g.cols) * g.W
                assert (flip.in_memory(w.numpy(), f) == upright[y:y + g.H, x:x + g.W]).all(), (f, i)
                seen[y:y + g.H, x:x + g.W] += 1
        assert (seen == 1).all()
    with pytest.raises(ValueError):
        tiles.encode_frame(None, mem, tile, flip=[1, 2])
    with pytest.raises(ValueError):
        tiles.decode_frame(None, [], mem, flip=5)
