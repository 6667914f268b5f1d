"""CPU: tests/levels.py — the prefixes that stop a decode at every level, the batches made of them, and that the batches
and layouts of tests/test_levels_gpu.py reach every kernel family they are there for (wide, LDS tail, general), as the
layouts' own offsets and strides decide it.  The oracle alone; no device."""
import pytest

import deep
import levels as Lv
import orc
import test_levels_gpu as G

depths = pytest.mark.parametrize("is16", [False, True], ids=["u8", "u16"])
colours = pytest.mark.parametrize("Cn", [1, 3], ids=["gray", "rgb"])
shapes = pytest.mark.parametrize("wh", Lv.SHAPES, ids=G.wh_ids)


def test_the_geometry_is_the_one_the_shapes_were_chosen_for():
    assert Lv.sizes(263, 135)[::-1] == [(263, 135), (132, 68), (66, 34), (33, 17), (17, 9), (9, 5)]
    assert Lv.sizes(511, 259)[::-1][:4] == [(511, 259), (256, 130), (128, 65), (64, 33)]
    assert Lv.sizes(520, 264)[::-1][:4] == [(520, 264), (260, 132), (130, 66), (65, 33)]
    assert Lv.sizes(256, 256)[::-1] == [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16), (8, 8), (4, 4)]


def test_family_restates_the_documented_rule():
    assert Lv.family(132, 68, True) == "wide" and Lv.family(132, 68, False) == "general"
    assert Lv.family(128, 65, True) == "wide" and Lv.family(64, 65, True) == "wide" and Lv.family(68, 8, True) == "wide"
    assert Lv.family(130, 66, True) == "general" and Lv.family(65, 33, True) == "general" and Lv.family(263, 135, True) == "general"
    assert Lv.family(64, 64, True) == "tail" and Lv.family(64, 33, False) == "tail" and Lv.family(33, 17, True) == "tail"


def same_missing_below(W, H):
    """The levels below which the longest prefix of a level may leave the same missing[] as the shortest: levels 0 and 1 of
    263x135 (pictures of 17x9 and 33x17) are a byte or two of some streams, within one bit plane of one ring.  From level 2 on,
    and at every level of the other shapes, the two differ in every picture, which is asserted."""
    return 2 if (W, H) == (263, 135) else 0


@depths
@colours
@shapes
def test_every_level_has_a_prefix(wh, Cn, is16):
    """The shortest prefix of level l decodes to level l and to the picture of heights / widths[l + 1]; one byte less stops a
    level earlier or is unreadable; the longest prefix of the level has the same level and another missing[]."""
    W, H = wh
    g = orc.geometry(W, H)
    for i in (0, 1, 7):
        data = Lv.stream(W, H, Cn, is16, i)
        assert orc.decode_stage(data, W, H, Cn)[1] == g.levels - 1
        for l in range(g.levels):
            p = Lv.prefix_for_level(data, W, H, Cn, l)
            _, level, missing, _ = orc.decode_stage(p, W, H, Cn)
            assert level == l, (i, l)
            assert Lv.level_at(data, W, H, Cn, len(p) - 1) in (l - 1, -2), (i, l)
            pic = deep.deep_decode(p, W, H, Cn, Lv.M16) if is16 else orc.decode(p)
            assert pic.shape == (g.heights[l + 1], g.widths[l + 1], Cn), (i, l)
            late = Lv.late_prefix(data, W, H, Cn, l)
            _, late_level, late_missing, _ = orc.decode_stage(late, W, H, Cn)
            assert len(late) > len(p) and late_level == l, (i, l)
            if l >= same_missing_below(W, H):
                assert late_missing.tolist() != missing.tolist(), (i, l)


@depths
@colours
@shapes
def test_the_batches_are_what_the_plan_says(wh, Cn, is16):
    """Every row of every case decodes (on the oracle) to the size the plan gives it — which is what the family counts below rest on."""
    W, H = wh
    S = Lv.sizes(W, H)
    n = 3
    plan = Lv.plan(W, H, n)
    cases = Lv.level_cases(W, H, Cn, is16, n)
    assert [c[0] for c in cases] == [p[0] for p in plan] and len(cases) == 3 * Lv.levels_of(W, H) + 5
    for (name, stops, cap), (_, rows, pixels_max) in zip(plan, cases):
        assert len(rows) == n and (pixels_max < 0) == (cap is None)
        assert deep.levels_max(W, H, pixels_max) == (-1 if cap is None else cap)
        for stop, row in zip(stops, rows):
            k = Lv.size_index(W, H, stop)
            level = orc.decode_stage(row, W, H, Cn, pixels_max)[1]
            if cap is None:
                assert level == k - 1, (name, stop)
            else:   # (at most the cap's size: levels.size_index)
                assert level <= min(k, cap) - 1, (name, stop)
            if name.startswith(("cap", "stairs", "one short")):
                pic = deep.deep_decode(row, W, H, Cn, Lv.M16, pixels_max) if is16 else orc.decode(row, pixels_max)
                assert pic.shape[:2] == S[level + 1][::-1], (name, stop)
    late = dict((c[0], c[1]) for c in cases)
    for l in range(Lv.levels_of(W, H)):   # one level, the rows' missing[] differ: a part that is not uniform, of equal sizes
        a, b = [orc.decode_stage(r, W, H, Cn) for r in late["stop %d late" % l][:2]]
        assert a[1] == b[1] == l and (l < same_missing_below(W, H) or a[2].tolist() != b[2].tolist()), l


@pytest.mark.parametrize("n", [8, 12, 24])
@pytest.mark.parametrize("wh", Lv.SHAPES, ids=G.wh_ids)
def test_stairs_hold_every_size(wh, n):
    """The batch sizes of the mixed tests: every level, and the whole stream, at least once; no decoder part is uniform."""
    W, H = wh
    T = Lv.levels_of(W, H)
    plan = dict((name, (stops, cap)) for name, stops, cap in Lv.plan(W, H, n))
    stops, cap = plan["stairs"]
    ks = [Lv.size_index(W, H, s) for s in stops]
    assert cap is None and set(ks) == set(range(1, T + 1)), ks   # (size index 0, the root alone, is what "cap 0" decodes)
    for part in deep.decoder_parts(n):
        assert len(set(ks[i] for i in part)) > 1, (n, list(part))
    stops, cap = plan["stairs capped"]
    assert cap == T // 2 and min(ks) < cap < max(ks) and [Lv.size_index(W, H, s) for s in stops] == ks   # the same rows: below and above the cap
    for name, at in (("one short", n - 1), ("short first", 0)):
        stops, cap = plan[name]
        ks = [Lv.size_index(W, H, s) for s in stops]
        assert cap is None and ks[at] == T - 1 and all(k == T for i, k in enumerate(ks) if i != at)


# ---- the families the GPU tests reach -----------------------------------------------------------------------------------------

def reached(sink, W, H, is16, floats=False):
    """{(family, ow, oh)} of a sink of tests/test_levels_gpu.py at a shape, by its layout's own offset and strides."""
    make = G.FLOAT_LAYOUTS[sink][1] if floats else G.VIEWS[sink][1]
    L = make(W, H)
    names = G.SMALL_CASES if (W, H) in G.SMALL else None
    return Lv.families(W, H, L.n, Lv.on_grid(L, is16, floats), names)


def dense_reached(W, H, Cn, n):
    size = W * H * Cn
    stride = G.P.up4(size) + 8 if n > 1 else size
    names = G.SMALL_CASES if (W, H) in G.SMALL else None
    return Lv.families(W, H, n, stride % Lv.QUAD == 0, names)


# the sinks whose windows lie on the quad grid at every shape: (sink, deep pixels too, float)
WIDE_SINKS = [("quad-gray", True, False), ("quad-rgb", True, False), ("nchw-quad", True, False), ("rgbx", False, False), ("bgrx", False, False),
              ("gray-quad", True, True), ("nchw-quad", True, True)]
SMALL_WIDE_SINKS = [("grid-gray", True, False), ("grid-rgb", True, False), ("nchw-8", True, False), ("gray-grid", True, True)]
GENERAL_SINKS = [("stack-gray", False), ("stack-rgb", False), ("gray-step2", False), ("rgb-grid", True)]


def test_every_family_is_reached_where_the_size_changes_it():
    """If a layout moved off the quad grid, its wide cases would silently become general ones: each is asserted here."""
    for sink, deep16, floats in WIDE_SINKS:
        assert sink in (G.FLOATS if floats else G.VIEWS), sink
        for is16 in (False, True) if deep16 else (False,):
            where = (sink, is16, floats)
            # general whole, wide reduced
            got = reached(sink, 263, 135, is16, floats)
            assert {("general", 263, 135), ("wide", 132, 68), ("general", 66, 34), ("tail", 33, 17), ("tail", 17, 9)} <= got, (where, got)
            # wide with only H above the tail (128x65), the tail from a width of 64
            got = reached(sink, 511, 259, is16, floats)
            assert {("general", 511, 259), ("wide", 256, 130), ("wide", 128, 65), ("tail", 64, 33), ("tail", 16, 9)} <= got, (where, got)
    for sink, deep16, floats in SMALL_WIDE_SINKS:
        assert sink in (G.SMALL_FLOATS if floats else G.SMALL_VIEWS), sink
        for is16 in (False, True):
            where = (sink, is16, floats)
            # wide whole, a strip edge at 260x132, general below it
            got = reached(sink, 520, 264, is16, floats)
            assert {("wide", 520, 264), ("wide", 260, 132), ("general", 130, 66), ("general", 65, 33), ("tail", 33, 17)} <= got, (where, got)
            # power-of-two squares: wide whole and reduced, the tail from 64x64
            got = reached(sink, 256, 256, is16, floats)
            assert {("wide", 256, 256), ("wide", 128, 128), ("tail", 64, 64), ("tail", 8, 8)} <= got, (where, got)
    # the stepped deep pixels, the gray step, the odd stack and interleaved float RGB never take the wide kernels: the general
    # path and the tail at every size
    for sink, floats in GENERAL_SINKS + [("rgbx", False), ("bgrx", False)]:
        is16 = sink in ("rgbx", "bgrx")
        for W, H in G.FULL:
            got = reached(sink, W, H, is16, floats)
            assert not any(f == "wide" for f, _, _ in got) and any(f == "general" for f, _, _ in got) and any(f == "tail" for f, _, _ in got), (sink, got)
    # dense slots: W * H * C apart a single picture; padded to the quad grid a batch of 8
    for Cn in (1, 3):
        assert ("wide", 132, 68) in dense_reached(263, 135, Cn, 8) and ("wide", 128, 65) in dense_reached(511, 259, Cn, 8)
        assert {("wide", 260, 132), ("general", 130, 66)} <= dense_reached(520, 264, Cn, 8)
        assert {("wide", 256, 256), ("wide", 128, 128), ("tail", 64, 64)} <= dense_reached(256, 256, Cn, 8)
        assert ("wide", 128, 128) in dense_reached(256, 256, Cn, 1) and ("wide", 260, 132) in dense_reached(520, 264, Cn, 1)
    assert not any(f == "wide" for f, _, _ in dense_reached(263, 135, 1, 1))   # (35505 samples a slot: off the grid)


def test_the_mixed_batches_reach_the_families_too():
    """The batches of the parts and switches tests (12 windows: grids on the quad grid at 520x264 and 256x256, the quad-grid stack and NCHW
    at every shape): a short stream among whole ones, and every size side by side."""
    for sink in G.PART_SINKS:
        for W, H in Lv.SHAPES:
            L = G.sized(sink, W, H, 12)
            got = Lv.families(W, H, 12, Lv.on_grid(L), G.MIXED)
            want = {(263, 135): {("wide", 132, 68), ("general", 263, 135)}, (511, 259): {("wide", 256, 130), ("wide", 128, 65), ("tail", 64, 33)},
                    (520, 264): {("wide", 520, 264), ("wide", 260, 132), ("general", 130, 66)},
                    (256, 256): {("wide", 256, 256), ("wide", 128, 128), ("tail", 64, 64)}}[W, H]
            if sink in ("quad-gray", "nchw-quad") or (W, H) in G.SMALL:
                assert want <= got, (sink, W, H, got)
            else:
                assert not any(f == "wide" for f, _, _ in got), (sink, W, H)
