"""CPU: the rectangles of the crop decode's kernel path (dwtx_crop_steps_of, dwtx_crop_origins, k_inv_level_roi in lift.hip)
as tests/crop.py restates them, and the case list of tests/test_crop_sweep_gpu.py held against that restatement.

The kernel path does not use dwtx_crop_plan, which tests/test_crop_cpu.py proves: it has one rectangle size per plane for
all pictures of a launch and another origin rule.  A lane that looks outside its LL rectangle reads 0, so a rectangle that
is too small gives a plausible wrong picture and no fault.  Here: the rectangles lie inside their bands and hold what the
kernel fetches, for every case of the GPU sweep and for every width, crop width and origin in one dimension; the numpy
inverse of tests/crop.py, fed those rectangles and poison everywhere else, gives the oracle's crop; the GPU cases reach every
class of rectangle the kernel's edge arithmetic tells apart; and the sweep's pictures tell neighbouring origins apart.
Nothing here needs a device."""
import functools

import numpy as np
import pytest

import crop
import orc
from test_crop_cpu import pyramid

GROUPS = crop.sweep_groups()


def case_id(c):
    return "%dx%dx%d %dx%d" % (c.W, c.H, c.Cn, c.cw, c.ch)


def axes_of(origins):
    """The rectangles are made per axis: the distinct x and y origins of a list -> two arrays (every bound below is one axis')"""
    return np.array(sorted({x for x, _ in origins})), np.array(sorted({y for _, y in origins}))


def check_coverage(S, x0, y0, what):
    """x0, y0: arrays of origins (of equal length, or one of them a single origin)"""
    xs, ys = crop.kernel_origins(S, x0, y0)
    assert S.tail_from <= S.T and all(S.w[t] == S.ws[t] and S.h[t] == S.hs[t] for t in range(max(S.tail_from, 1), S.T + 1)), what
    for t in range(S.T + 1):
        assert 1 <= S.w[t] <= S.ws[t] and 1 <= S.h[t] <= S.hs[t], (what, t)
        # the rectangle of plane t — the destination of step t, the source of step t - 1 — lies inside the plane
        assert (xs[t] >= 0).all() and (xs[t] + S.w[t] <= S.ws[t]).all(), (what, t)
        assert (ys[t] >= 0).all() and (ys[t] + S.h[t] <= S.hs[t]).all(), (what, t)
    for t in range(S.tail_from):
        k_lo, k_hi, j_lo, j_hi = crop.kernel_reads(S, xs, ys, t)
        bad = (k_lo < xs[t + 1]) | (k_hi >= xs[t + 1] + S.w[t + 1])
        assert not bad.any(), (what, t, "x", np.broadcast_to(x0, bad.shape)[bad][:5])
        bad = (j_lo < ys[t + 1]) | (j_hi >= ys[t + 1] + S.h[t + 1])
        assert not bad.any(), (what, t, "y", np.broadcast_to(y0, bad.shape)[bad][:5])
        # and the launch's grid reaches every pair: `pairs_x = a.dw / 2 + 1` strips' worth, whatever the origin's parity
        kA, kB = crop.pair_range(xs[t], S.w[t])
        jA, jB = crop.pair_range(ys[t], S.h[t])
        assert (kB - kA <= S.w[t] // 2 + 1).all() and (jB - jA <= S.h[t] // 2 + 1).all(), (what, t)


@pytest.mark.parametrize("name", list(GROUPS))
def test_kernel_rectangles_hold_what_the_kernel_reads(name):
    for c in GROUPS[name]:
        for S, origins in c.launches():
            x0, y0 = axes_of(origins)
            check_coverage(S, x0, y0[:1], case_id(c))
            check_coverage(S, x0[:1], y0, case_id(c))


@pytest.mark.parametrize("H", [None, 8], ids=["square", "thin"])
def test_kernel_rectangles_in_one_dimension(H):
    """every width 8 .. 200, every crop width, every origin: beside an equal side (the levels a square has) and beside a side of
    8 (one step, and above 64 columns no tail: tail_from == T)"""
    for W in range(8, 201):
        for cw in range(1, W + 1):
            S = crop.kernel_steps(W, H or W, cw, 1)
            check_coverage(S, np.arange(W - cw + 1), np.zeros(1, dtype=np.int64), (W, cw))


def test_restated_levels_are_the_oracles():
    """kernel_steps' planes are orc.geometry's levels, counted the other way round"""
    for W, H in sorted({(c.reduced or (c.W, c.H)) for cases in GROUPS.values() for c in cases} | {(c.W, c.H) for cases in GROUPS.values() for c in cases}):
        S, g = crop.kernel_steps(W, H, 1, 1), orc.geometry(W, H)
        assert S.T == g.levels
        assert [(S.ws[t], S.hs[t]) for t in range(S.T + 1)] == [(g.widths[S.T - t], g.heights[S.T - t]) for t in range(S.T + 1)]


# ---- the numpy inverse on the kernel's rectangles -----------------------------------------------------------------------------

def check_plans_agree(W, H, cw, ch, origins):
    pyr, want = pyramid(W, H)
    S = crop.kernel_steps(W, H, cw, ch)
    for x0, y0 in origins:   # (one call per origin: the sizes are shared, the rectangles are not)
        rects = crop.kernel_rects(S, *crop.kernel_origins(S, x0, y0))
        got = crop.windowed_inverse(pyr, x0, y0, cw, ch, rects)
        assert (got == want[y0:y0 + ch, x0:x0 + cw]).all(), (W, H, cw, ch, x0, y0)


def test_kernel_rectangles_invert_to_the_oracles_crop_at_every_origin():
    check_plans_agree(70, 67, 9, 7, crop.every_origin(70, 67, 9, 7))


@pytest.mark.parametrize("wh", crop.THIN, ids=lambda wh: "%dx%d" % wh)
def test_kernel_rectangles_invert_to_the_oracles_crop_on_thin_shapes(wh):
    W, H = wh
    for cw, ch in ((min(7, W), min(5, H)), (1, 1), (W - 1, H - 1)):
        check_plans_agree(W, H, cw, ch, crop.sampled_origins(W, H, cw, ch))


def test_a_short_kernel_rectangle_is_noticed():
    """the check can fail: one column or row less on the windowed plane, and poison reaches the crop"""
    W, H, cw, ch, x0, y0 = 70, 67, 9, 7, 30, 28
    pyr, want = pyramid(W, H)
    S = crop.kernel_steps(W, H, cw, ch)
    assert S.tail_from == 1
    rects = crop.kernel_rects(S, *crop.kernel_origins(S, x0, y0))
    l = len(rects) - 1   # the picture's own rectangle: one sample short on either axis
    x, y, w, h = rects[l]
    for short in ((x, y, w - 1, h), (x, y, w, h - 1), (x + 1, y, w - 1, h), (x, y + 1, w, h - 1)):
        bad = rects[:l] + [short]
        assert not (crop.windowed_inverse(pyr, x0, y0, cw, ch, bad) == want[y0:y0 + ch, x0:x0 + cw]).all(), short


# ---- what the GPU cases reach --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reached():
    """-> ({(plane t, axis, word)} over the route 1 cases, {(plane t, axis, word)} of the LIFT_ROWS 4 cases, {shape word},
    {test id: sorted words}) from the restatement"""
    all_, rows4, shapes, by_id = set(), set(), set(), {}
    for name, cases in GROUPS.items():
        mine = set()
        for c in cases:
            if c.route != 1:
                continue
            for S, origins in c.launches():
                if S.tail_from == S.T and S.tail_from > 0:
                    shapes.add("no tail")
                first = S.tail_from - 1   # the first windowed step that runs: the coarsest one, on the LDS tail's output
                if 0 <= first and S.tail_from < S.T and min(S.ws[first], S.hs[first]) <= crop.TAIL_MAX:
                    shapes.add("thin first level")
                x0, y0 = axes_of(origins)
                for pts, axis in (([(x, int(y0[0])) for x in x0], "x"), ([(int(x0[0]), y) for y in y0], "y")):
                    for x, y in pts:
                        xs, ys = crop.kernel_origins(S, int(x), int(y))
                        for t in range(S.tail_from):
                            got = {(t, a, w) for a, w in crop.classes(S, xs, ys, t, c.rows_per_wave) if a == axis}
                            mine |= got
                            if c.rows_per_wave == 4:
                                rows4 |= got
        all_ |= mine
        by_id[name] = sorted(mine)
    return all_, rows4, shapes, by_id


def test_gpu_cases_reach_every_class_of_rectangle():
    all_, rows4, shapes, by_id = reached()
    for name, words in by_id.items():   # what each GPU case reaches: pytest -s, or a failure's captured output
        print("%s: %s" % (name, " ".join("%d%s:%s" % w for w in words)))
    levels = sorted({t for t, _, _ in all_})
    assert levels == [0, 1, 2]
    want = set()
    for t in levels:
        for axis in "xy":
            want |= {(t, axis, w) for w in ("even", "odd", "narrow", "band", "frozen", "thawed")}
            if t >= 1:   # (plane 0's origin is the caller's: dwtx_crop_origins moves none)
                want |= {(t, axis, w) for w in ("at0", "far", "free")}
        if t <= 1:
            want |= {(t, "x", "strips1"), (t, "x", "strips2")}
    assert not want - all_, sorted(want - all_)
    assert {(0, "y", "waves2"), (1, "y", "waves2")} <= rows4, sorted(rows4)
    assert shapes == {"no tail", "thin first level"}


def test_every_gpu_call_shares_one_size_and_fits_its_picture():
    total = 0
    for name, cases in GROUPS.items():
        for c in cases:
            W, H = c.reduced or (c.W, c.H)
            assert c.origins and 1 <= c.cw <= c.W and 1 <= c.ch <= c.H, name
            assert all(0 <= x <= W - c.cw and 0 <= y <= H - c.ch for x, y in c.origins), name
            assert len(set(c.origins)) == len(c.origins) <= crop.GROUP_MAX, name
            total += len(c.origins)
    assert total > 60000


# ---- the pictures --------------------------------------------------------------------------------------------------------------

def pictures():
    seen = {}
    for cases in GROUPS.values():
        for c in cases:
            seen.setdefault((c.W, c.H, c.Cn, c.reduced), c)
    return list(seen.values())


@pytest.mark.parametrize("c", pictures(), ids=lambda c: "%dx%dx%d%s" % (c.W, c.H, c.Cn, "-reduced" if c.reduced else ""))
def test_pictures_tell_neighbouring_origins_apart(c):
    """a result shifted by one sample must not pass: 7 x 5 crops (the thin shapes' size) one column or one row apart differ in
    more than half their samples, at every origin"""
    pic = crop.sweep_stream(c)[1]
    cw, ch = min(7, c.W), min(5, c.H)
    win = np.lib.stride_tricks.sliding_window_view(pic, (ch, cw), axis=(0, 1))   # [y0, x0, channel, ch, cw]
    half = ch * cw * c.Cn / 2
    assert ((win[:, 1:] != win[:, :-1]).sum(axis=(2, 3, 4)) > half).all()
    assert ((win[1:] != win[:-1]).sum(axis=(2, 3, 4)) > half).all()
