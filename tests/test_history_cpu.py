"""CPU: the conditions that keep tests/test_history_gpu.py honest, for every scenario of tests/history.py — with the oracle
alone, no device.

A target that is decoded after dirt proves something only if a stale word would be a WRONG word: the dirt shares at most 1 %
of its coefficients with the target (coincidence), noise dirt has more bit planes than every target that is not noise itself
on every channel (a segment the target leaves empty was full before), and no scratch slot grows during the target call — a
dirt call of the target's family has at least its batch, its samples per image and its stream stride — so that the stale
bytes are the dirt's and not a fresh allocation's.  These are conditions, not measurements: a pair that misses one gets
another seed or shape in tests/history.py, never a wider bound here."""
import numpy as np
import pytest

import history as Hs
import orc

GROUPS = sorted({g for g, _ in Hs.SCENARIOS})
_seen = {}


def _key(x):
    return x if isinstance(x, bytes) else id(x)


def test_every_group_has_scenarios_and_every_name_is_its_own():
    assert GROUPS == ["broken", "crop", "decode", "encode", "index", "sink", "switch"]
    names = [s.name for _, s in Hs.SCENARIOS]
    assert len(set(names)) == len(names)


def test_coincidence_measures_what_it_says():
    p = orc.synth(72, 68, 3, 1, 0)
    assert Hs.coincidence(p, p) == 1.0
    assert Hs.coincidence(p, orc.encode(p)[0]) == 1.0        # a whole stream is its picture
    flat = Hs.flat_picture(72, 68, 1)
    lin = Hs.lin_of(flat)
    assert Hs.coincidence(flat, np.zeros_like(flat)) == float((lin == 0).mean()) > 0.98   # all but the root image
    assert Hs.coincidence(p, orc.encode(p)[0][:7]) == 0.0    # unreadable: nothing is written
    # a prefix: what the oracle decodes of it, zeros where it decodes nothing
    short = Hs.V.cut(*orc.encode(p))
    r = orc.decode_stage(short, 72, 68, 3)
    assert r is not None and abs(Hs.coincidence(p, short) - float((Hs.lin_of(p) == r[0]).mean())) == 0.0


@pytest.mark.parametrize("shape", Hs.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_kind_0_is_unfit_as_dirt_and_noise_is_not(shape):
    """what an unwritten coefficient of a target would read is most often 0: dirt must not hold zeros"""
    W, H, Cn = shape
    assert (Hs.lin_of(orc.synth(W, H, Cn, Hs.DIRT_SEED, 0)) == 0).mean() > 0.10
    for depth in (8, 4095, 65535):
        assert (Hs.lin_of(Hs.dirt_picture(W, H, Cn, "noise", depth, 0)) == 0).mean() < Hs.COINCIDENCE_MAX


@pytest.mark.parametrize("shape", Hs.SHAPES + [(135, 263, 1), (135, 263, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_deep_dirt_has_the_planes_it_is_there_for(shape):
    """maxval 65535: 16 bit planes on some channel of every picture — coefficients past 15 bits, which keep a part out of the 16-bit
    ring planes — and never 17, which the decoder refuses; maxval 4095: past the 11 an 8-bit picture can reach"""
    W, H, Cn = shape
    for i in range(Hs.DIRT_N):
        assert max(Hs.planes_of(Hs.dirt_stream(W, H, Cn, "noise", 65535, i))) == 16, i
        assert 12 <= max(Hs.planes_of(Hs.dirt_stream(W, H, Cn, "noise", 4095, i))) <= 15, i


@pytest.mark.parametrize("group", GROUPS)
def test_dirt_and_target_share_at_most_one_coefficient_in_a_hundred(group):
    worst = 0.0
    for s in Hs.group(group):
        for dpix, _, _, what, _, _ in Hs.pairs(s):
            key = ("c", id(dpix), _key(what))
            if key not in _seen:
                _seen[key] = Hs.coincidence(dpix, what)
            worst = max(worst, _seen[key])
            assert _seen[key] <= Hs.COINCIDENCE_MAX, (s.name, _seen[key])
    print(group, "largest coincidence", worst)


@pytest.mark.parametrize("group", GROUPS)
def test_noise_dirt_has_more_planes_than_the_target_on_every_channel(group):
    checked = 0
    for s in Hs.group(group):
        for _, dirt_is_noise, dstream, _, tstream, target_is_noise in Hs.pairs(s):
            tp = Hs.planes_of(tstream)
            if not dirt_is_noise or target_is_noise or tp is None:
                continue
            dp = Hs.planes_of(dstream)
            assert min(dp) > max(tp), (s.name, dp, tp)
            checked += 1
    assert checked or group == "none"
    print(group, checked, "pairs")


@pytest.mark.parametrize("group", GROUPS)
def test_no_slot_grows_during_the_target_call(group):
    fresh = 0
    for s in Hs.group(group):
        calls = Hs.calls_of(s)
        if isinstance(s.target, Hs.EncTarget):
            assert len(Hs.encoder_pictures(s.target.W, s.target.H, s.target.Cn, s.target.content)[0]) == s.target.n
        if not calls:   # a fresh context's first call: everything grows, nothing is stale — the one exemption
            assert s.hist == "none"
            fresh += 1
            continue
        assert s.family == ("encode" if isinstance(s.target, Hs.EncTarget) else "decode")
        assert any(Hs.HOWS[cl.how] == s.family and Hs.covers(cl, s.target) for cl in calls), s.name
        assert all(cl.n == Hs.DIRT_N for cl in calls), s.name
    print(group, fresh, "scenarios without a history")


def test_targets_and_dirt_never_share_a_seed():
    assert Hs.DIRT_SEED >= 9000
    for _, s in Hs.SCENARIOS:
        assert s.target.n <= 5   # the targets' pictures are seeds 0 .. n - 1 (tests/test_views_gpu.py picture(), tests/levels.py stream())


def test_the_targets_reach_the_paths_they_are_named_for():
    import deep
    import levels

    assert levels.sizes(263, 135)[levels.levels_of(263, 135) - 1] == (132, 68)
    assert deep.levels16(256, 256) and not deep.levels16(263, 135)
    assert levels.family(64, 64, True) == "tail" and levels.family(72, 68, True) == "wide" and levels.family(263, 135, True) == "general"
    for t in (Hs.target(Hs.GENERAL_RGB, 5, "broken"), Hs.target(Hs.WIDE_GRAY, 5, "broken")):
        rows = Hs.rows_of(t)
        got = [orc.decode_stage(r, t.W, t.H, t.Cn) for r in rows]
        T = levels.levels_of(t.W, t.H)
        assert got[3] is None and [g[1] for g in got if g is not None] == [T - 1, T - 2, got[2][1], T - 1]
        assert got[2][2].any()   # the cut stream misses planes
    for shape in Hs.SHAPES:   # sparse pictures come out whole (a uniform part, the fused route) and most of their finest tiles are empty
        t = Hs.target(shape, 5, "sparse")
        T, g = levels.levels_of(t.W, t.H), orc.geometry(t.W, t.H)
        for r in Hs.rows_of(t):
            lin, level, missing, planes = orc.decode_stage(r, t.W, t.H, t.Cn)
            assert level == T - 1 and not missing.any() and 1 <= max(planes) <= 6
            assert (lin[:, g.pixels[T - 1]:] != 0).mean() < 0.01
    for t in (Hs.target(Hs.GENERAL_RGB, 5, "mixed"), Hs.target(Hs.WIDE_GRAY, 5, "mixed")):
        rows = Hs.rows_of(t)
        assert Hs.planes_of(rows[0]) == (0,) * t.Cn and max(Hs.planes_of(rows[1])) == 6
