"""CPU: dwtx_tile_groups (include/dwtx.h) against a restatement of its rule in a few lines of Python: the groups
cover the frame exactly once, and every tile side lies in [8, tile + 7].  Host arithmetic only, no compute calls."""
import itertools

import pytest

ERR_ARG = -3
SIDES = [8, 15, 16, 100, 4096, 4103, 4104, 40000, 70000]
TILES = [8, 64, 4096]


def axis(side, tile):
    """The tile sizes along one axis, first to last."""
    if side < tile:
        return [side]
    full, rem = divmod(side, tile)
    if rem == 0:
        return [tile] * full
    if rem >= 8:
        return [tile] * full + [rem]
    return [tile] * (full - 1) + [tile + rem]


def rectangles(groups):
    """(x, y, w, h) of every tile of every group."""
    out = []
    for g in groups:
        for r in range(g.rows):
            for c in range(g.cols):
                out.append((g.x0 + c * g.W, g.y0 + r * g.H, g.W, g.H))
    return out


def expected(W, H, tile):
    xs, ys = axis(W, tile), axis(H, tile)
    out, y = [], 0
    for h in ys:
        x = 0
        for w in xs:
            out.append((x, y, w, h))
            x += w
        y += h
    return out


@pytest.mark.parametrize("tile", TILES)
def test_groups_tile_the_frame_exactly_once(tile):
    import dwt_amd

    mixed = [(4103, 8), (15, 70000), (40000, 100), (100, 4104), (16, 4096), (70000, 4103)]
    for W, H in [(s, s) for s in SIDES] + mixed:
        if (W // tile + 1) * (H // tile + 1) > 400000:   # (a Python list of that many rectangles proves nothing more)
            continue
        groups = dwt_amd.tile_groups(W, H, tile)
        assert 1 <= len(groups) <= 4, (W, H, tile)
        for g in groups:
            assert 8 <= g.W <= tile + 7 and 8 <= g.H <= tile + 7 and g.cols >= 1 and g.rows >= 1, (W, H, tile)
        got = rectangles(groups)
        want = expected(W, H, tile)
        assert sorted(got) == sorted(want), (W, H, tile)
        assert sum(w * h for _, _, w, h in got) == W * H
        # interior first, corner last: the first group starts at the origin, x0 / y0 never decrease
        assert (groups[0].x0, groups[0].y0) == (0, 0)
        assert [(g.y0, g.x0) for g in groups] == sorted((g.y0, g.x0) for g in groups)


def test_large_frames_by_counts():
    """Frames whose tiles are too many to list: the groups' counts and sizes against the rule, per axis."""
    import dwt_amd

    for W, H, tile in itertools.product([40000, 70000, 4103], [40000, 70000, 8], [8, 64, 4096]):
        groups = dwt_amd.tile_groups(W, H, tile)
        xs, ys = axis(W, tile), axis(H, tile)
        cols = {}
        rows = {}
        for g in groups:
            cols[(g.x0, g.W)] = g.cols
            rows[(g.y0, g.H)] = g.rows
            assert 8 <= g.W <= tile + 7 and 8 <= g.H <= tile + 7
        assert sum(w * c for (_, w), c in cols.items()) == W and sum(cols.values()) == len(xs)
        assert sum(h * r for (_, h), r in rows.items()) == H and sum(rows.values()) == len(ys)
        assert sorted(set(xs)) == sorted({w for _, w in cols}) and sorted(set(ys)) == sorted({h for _, h in rows})
        assert sum(g.cols * g.rows * g.W * g.H for g in groups) == W * H


@pytest.mark.parametrize("W,H,tile", [(100, 100, 0), (100, 100, 4), (100, 100, 10), (100, 100, 66), (100, 100, -8),
                                      (7, 100, 8), (100, 7, 8), (100, 100, 32772)])
def test_bad_plan_is_refused(W, H, tile):
    import dwt_amd
    from dwt_amd import _lib

    out = (dwt_amd.TileGroup * 4)()
    assert _lib.load().dwtx_tile_groups(W, H, tile, out) == ERR_ARG
    assert _lib.load().dwtx_last_error()
    with pytest.raises(dwt_amd.DwtxError):
        dwt_amd.tile_groups(W, H, tile)
