"""CPU: the plan of a crop decode (dwtx_crop_plan, include/dwtx.h) — which rectangle of every level a window of the picture
needs.  tests/crop.py restates the plan and undoes the transform with nothing but the planned rectangles (everything else
is poison); the result must be the oracle's inverse, sliced, and the library must return exactly the restated rectangles.
Every comparison is exact; nothing here needs a device."""
import functools

import numpy as np
import pytest

import crop
import orc

ERR_ARG = -3
EXHAUSTIVE = [(37, 53), (16, 9)]
SAMPLED = [(8, 8), (64, 64), (72, 68), (130, 67), (263, 135)]
CROPS = [(1, 1), (5, 3), (20, 31), None]   # None: the whole picture


@functools.lru_cache(maxsize=None)
def pyramid(W, H):
    """A random int32 pyramid and the oracle's inverse of it"""
    rng = np.random.default_rng(W * 1000 + H)
    pyr = rng.integers(-2000, 2000, (H, W), dtype=np.int32)
    return pyr, orc.inverse(pyr[:, :, None])[:, :, 0]


def crops_of(W, H):
    return [(W, H) if c is None else c for c in CROPS if c is None or (c[0] <= W and c[1] <= H)]


def library_plan(W, H, x0, y0, cw, ch):
    import dwt_amd

    return dwt_amd.crop_plan(W, H, x0, y0, cw, ch)


def check(W, H, origins_of):
    pyr, want = pyramid(W, H)
    for cw, ch in crops_of(W, H):
        for x0, y0 in origins_of(cw, ch):
            rects = crop.plan(W, H, x0, y0, cw, ch)
            got = crop.windowed_inverse(pyr, x0, y0, cw, ch, rects)
            assert (got == want[y0:y0 + ch, x0:x0 + cw]).all(), (W, H, x0, y0, cw, ch)
            assert library_plan(W, H, x0, y0, cw, ch) == rects, (W, H, x0, y0, cw, ch)


@pytest.mark.parametrize("wh", EXHAUSTIVE + SAMPLED, ids=lambda wh: "%dx%d" % wh)
def test_numpy_inverse_is_the_oracles(wh):
    """the helper the other tests stand on: crop.inverse on a whole pyramid is orc.inverse"""
    pyr, want = pyramid(*wh)
    assert (crop.inverse(pyr) == want).all()


def test_poison_is_noticed():
    """a plan that keeps one column or row too few on one level does not pass: the check can fail.  (A crop that ends on an
    even sample: its last odd sample needs the pair beyond it.  One that ends on an odd one keeps a column it could do without.)"""
    W, H = 37, 53
    pyr, want = pyramid(W, H)
    x0, y0, cw, ch = 9, 11, 21, 31
    rects = crop.plan(W, H, x0, y0, cw, ch)
    assert (crop.windowed_inverse(pyr, x0, y0, cw, ch, rects) == want[y0:y0 + ch, x0:x0 + cw]).all()
    l = len(rects) - 2
    for short in ((rects[l][0] + 1, rects[l][1], rects[l][2] - 1, rects[l][3]), (rects[l][0], rects[l][1], rects[l][2] - 1, rects[l][3]),
                  (rects[l][0], rects[l][1] + 1, rects[l][2], rects[l][3] - 1), (rects[l][0], rects[l][1], rects[l][2], rects[l][3] - 1)):
        bad = rects[:l] + [short] + rects[l + 1:]
        assert not (crop.windowed_inverse(pyr, x0, y0, cw, ch, bad) == want[y0:y0 + ch, x0:x0 + cw]).all(), short


@pytest.mark.parametrize("wh", EXHAUSTIVE, ids=lambda wh: "%dx%d" % wh)
def test_plan_every_origin(wh):
    W, H = wh
    check(W, H, lambda cw, ch: [(x, y) for y in range(H - ch + 1) for x in range(W - cw + 1)])


@pytest.mark.parametrize("wh", SAMPLED, ids=lambda wh: "%dx%d" % wh)
def test_plan_sampled_origins(wh):
    W, H = wh
    check(W, H, lambda cw, ch: crop.sampled_origins(W, H, cw, ch))


def test_sampled_origins_cover_parities_edges_and_corners():
    o = crop.sampled_origins(263, 135, 5, 3)
    assert {(x & 1, y & 1) for x, y in o} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(0, 0), (258, 0), (0, 132), (258, 132)} <= set(o)


def test_plan_shape():
    """root first, the crop itself last, every rectangle inside its band"""
    W, H = 263, 135
    g = orc.geometry(W, H)
    rects = library_plan(W, H, 31, 17, 200, 100)
    assert len(rects) == g.levels + 1 and rects[-1] == (31, 17, 200, 100)
    for l, (x0, y0, w, h) in enumerate(rects):
        assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= g.widths[l] and y0 + h <= g.heights[l]


@pytest.mark.parametrize("args", [(263, 135, 0, 0, 264, 10), (263, 135, 0, 0, 10, 136), (263, 135, 0, 0, 0, 10), (263, 135, 0, 0, 10, 0),
                                  (263, 135, -1, 0, 10, 10), (263, 135, 0, -1, 10, 10), (263, 135, 254, 0, 10, 10), (263, 135, 0, 126, 10, 10),
                                  (7, 135, 0, 0, 1, 1), (263, 7, 0, 0, 1, 1), (32769, 16, 0, 0, 1, 1)])
def test_plan_refusals(args):
    import ctypes as C

    from dwt_amd import _lib

    out = (_lib.CropRect * (_lib.MAX_LEVELS + 1))()
    assert _lib.load().dwtx_crop_plan(*args, out) == ERR_ARG
    assert _lib.load().dwtx_crop_plan(263, 135, 0, 0, 10, 10, C.cast(None, C.POINTER(_lib.CropRect))) == ERR_ARG
