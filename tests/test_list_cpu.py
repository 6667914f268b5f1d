"""CPU: window lists (dwtx_view_list_check, include/dwtx.h) — what dwtx_encode_view_list and dwtx_decode_view_list accept
of one pointer per picture.  Host arithmetic only: the pointers are plain integers and are never dereferenced.

The decode's rule ("provably disjoint": two units a span apart, or in different columns of one pitch lattice) is held
against the brute-force sets of sample addresses: it may refuse lists that are disjoint — it is sufficient, not necessary —
but it must never accept one whose sets intersect."""
import random

import pytest

import dwt_amd

ERR_ARG = -3
BASE = 0x7F4000000000   # where the made-up windows lie


def check(ptrs, W, H, dst=True, **view):
    return dwt_amd.view_list_check(ptrs, W, H, dst=dst, **view)


def accepted(ptrs, W, H, **view):
    rc, text = check(ptrs, W, H, **view)
    assert (rc == 0) == (text == ""), (rc, text)
    assert rc in (0, ERR_ARG), (rc, text)
    return rc == 0


def addresses(p, W, H, channels, row_pitch, channel_stride, pixel_step):
    """the sample addresses (in samples) of the window at sample p, as dwtx_pixels reads and writes them"""
    step = 1 if channel_stride else (pixel_step or channels)
    cs = channel_stride or 1
    return [p + y * row_pitch + x * step + c * cs for y in range(H) for x in range(W) for c in range(channels)]


def intersect(ptrs, W, H, channels, row_pitch, channel_stride, pixel_step):
    seen = set()
    for p in ptrs:
        a = addresses(p, W, H, channels, row_pitch, channel_stride, pixel_step)
        if len(set(a)) != len(a) or not seen.isdisjoint(a):
            return True
        seen.update(a)
    return False


# ---- the rule against brute force -----------------------------------------------------------------------------------------

def random_list(rng, k):
    """2 to 5 units on the cells of a pitch lattice; in every second list one of them nudged by up to a row"""
    mode = ("gray", "rgb", "stepped", "planar")[k % 4]
    W, H = rng.randint(1, 6), rng.randint(1, 4)
    channels = 1 if mode == "gray" or (mode == "stepped" and rng.random() < 0.5) else 3
    pixel_step = channels + rng.randint(1, 2) if mode == "stepped" else 0
    row = W if mode == "planar" else (W - 1) * (pixel_step or channels) + channels
    cells_x, cells_y = rng.randint(2, 3), rng.randint(2, 3)
    pitch = cells_x * row + rng.randint(0, 2)
    units = rng.randint(2, 5)
    cells = [(cx, cy) for cy in range(cells_y) for cx in range(cells_x)]
    channel_stride = 0
    if mode == "planar":
        # a CHW frame (the planes of the whole lattice apart), an NCHW stack (a window's planes in three bands of their own),
        # or planes that lie anywhere
        how = rng.choice(("chw", "nchw", "any"))
        if how == "chw":
            channel_stride = cells_y * H * pitch
        elif how == "nchw":
            channel_stride = H * pitch
            cells = [(cx, 3 * cy) for cx, cy in cells]
        else:
            channel_stride = rng.randint(1, 2 * H * pitch)
        units = rng.randint(2, 3)
    rng.shuffle(cells)
    starts = [cy * H * pitch + cx * row for cx, cy in cells[:units]]
    if k % 2:
        i = rng.randrange(len(starts))
        starts[i] = max(0, starts[i] + rng.choice([-1, 1]) * rng.randint(1, row))
    return starts, W, H, dict(channels=channels, row_pitch=pitch, channel_stride=channel_stride, pixel_step=pixel_step)


def test_the_rule_never_accepts_lists_whose_samples_intersect():
    rng = random.Random(20260)
    N = 4000
    took = refused = wrong = 0
    for k in range(N):
        starts, W, H, view = random_list(rng, k)
        sample_bytes = (1, 2, 4)[k % 3]
        ok = accepted([BASE + s * sample_bytes for s in starts], W, H, sample_bytes=sample_bytes, **view)
        took += ok
        refused += not ok
        if ok and intersect(starts, W, H, **view):
            wrong += 1
            print("accepted although the windows intersect:", starts, W, H, view)
    print(f"{N} lists: {took} accepted, {refused} refused")
    assert wrong == 0
    assert took >= N // 20 and refused >= N // 20, (took, refused)


def test_the_undisturbed_lattice_is_accepted_in_any_order():
    rng = random.Random(7)
    for k in range(0, 400, 2):   # (the even lists are not nudged)
        starts, W, H, view = random_list(rng, k)
        if view["channel_stride"]:
            continue
        assert not intersect(starts, W, H, **view)
        assert accepted([BASE + s for s in starts], W, H, **view), (starts, W, H, view)


# ---- named layouts --------------------------------------------------------------------------------------------------------

W, H = 12, 10
FW, FH = 64, 40   # a frame, in pixels


def tiles(channels=1, step=0, cols=4, rows=3, x0=4, y0=2):
    """the tiles of a cols x rows grid in the frame, row by row: their first samples"""
    px = step or channels
    return [BASE + ((y0 + ty * H) * FW + x0 + tx * W) * px for ty in range(rows) for tx in range(cols)]


def layouts_taken():
    rng = random.Random(3)
    span = (H - 1) * W * 3 + W * 3
    allocs = [BASE + i * (span + 256 * rng.randint(1, 9)) for i in range(6)]
    rng.shuffle(allocs)
    grid = tiles(3)
    shuffled = grid[:]
    rng.shuffle(shuffled)
    boxes = [BASE + (y * FW + x) for x, y in ((0, 0), (W, 0), (2 * W + 3, 1), (0, H), (W + 1, H + 5), (40, 3 * H))]
    return [
        ("separate allocations in shuffled order", allocs, dict(channels=3)),
        ("a tile grid in a permuted order", shuffled, dict(channels=3, row_pitch=FW * 3)),
        ("a subset of a tile grid", grid[1::3] + grid[:1], dict(channels=3, row_pitch=FW * 3)),
        ("an NCHW stack listed per picture", [BASE + i * 3 * W * H for i in (2, 0, 1, 3)], dict(channels=3, channel_stride=W * H)),
        ("a CHW frame's tiles", tiles(1), dict(channels=3, row_pitch=FW, channel_stride=FW * FH)),
        ("boxes side by side and above one another", boxes, dict(channels=1, row_pitch=FW)),
        ("the RGB windows of an RGBA surface", tiles(3, 4), dict(channels=3, row_pitch=FW * 4, pixel_step=4)),
    ]


@pytest.mark.parametrize("name,ptrs,view", layouts_taken(), ids=[l[0] for l in layouts_taken()])
def test_layouts_that_are_accepted(name, ptrs, view):
    assert len(set(ptrs)) == len(ptrs)
    for sample_bytes in (1, 2, 4):
        scaled = [BASE + (p - BASE) * sample_bytes for p in ptrs]
        assert check(scaled, W, H, sample_bytes=sample_bytes, **view) == (0, ""), sample_bytes
        assert check(scaled, W, H, dst=False, sample_bytes=sample_bytes, **view) == (0, "")


def layouts_refused():
    """(name, pointers, view, whether the encode refuses them too)"""
    row, pitch = W * 3, FW * 3
    plane = (H - 1) * FW + W
    return [
        ("one pointer twice", [BASE, BASE + 4096, BASE], dict(channels=3), False),
        ("two windows less than a row apart", [BASE, BASE + row - 1], dict(channels=3, row_pitch=pitch), False),
        ("two windows pitch - row + 1 apart", [BASE, BASE + pitch - row + 1], dict(channels=3, row_pitch=pitch), False),
        ("planar planes closer than a plane", [BASE, BASE + 3 * FW * FH], dict(channels=3, row_pitch=FW, channel_stride=plane - 1), False),
        ("a NULL entry", [BASE, 0, BASE + 4096], dict(channels=3), True),
        ("a misaligned entry", [BASE, BASE + 4097], dict(channels=1, sample_bytes=2), True),
    ]


@pytest.mark.parametrize("name,ptrs,view,always", layouts_refused(), ids=[l[0] for l in layouts_refused()])
def test_layouts_that_are_refused_with_a_text(name, ptrs, view, always):
    rc, text = check(ptrs, W, H, **view)
    assert rc == ERR_ARG and text.strip(), name
    # the encode may read overlapping windows: it refuses only what it cannot address
    rc, text = check(ptrs, W, H, dst=False, **view)
    if always:
        assert rc == ERR_ARG and text.strip(), name
    else:
        assert (rc, text) == (0, ""), name


def test_the_bounds_themselves_are_accepted():
    row, pitch = W * 3, FW * 3
    span = (H - 1) * pitch + row
    for d in (row, pitch - row, span, 5 * pitch + row):
        assert check([BASE + d, BASE], W, H, channels=3, row_pitch=pitch) == (0, ""), d
    assert check([BASE + pitch, BASE], W, H, channels=3, row_pitch=pitch)[0] == ERR_ARG   # (one row down: the same columns)
    plane = (H - 1) * FW + W
    assert check([BASE, BASE + 3 * FW * FH], W, H, channels=3, row_pitch=FW, channel_stride=plane) == (0, "")


def test_counts_and_views_are_refused_as_the_calls_refuse_them():
    far = [BASE + i * 4096 for i in range(8)]
    assert check(far, 8, 8) == (0, "")
    for what, got in [
        ("no windows", check([], 8, 8)),
        ("a pitch below the row", check(far, 8, 8, channels=3, row_pitch=23)),
        ("two channels", check(far, 8, 8, channels=2, row_pitch=16)),
        ("a step below the channels", check(far, 8, 8, channels=3, pixel_step=2, row_pitch=64)),
        ("a maxval of 0 for a destination", check(far, 8, 8, sample_bytes=2, maxval=0)),
        ("a side of 0", check(far, 0, 8, row_pitch=8)),
    ]:
        assert got[0] == ERR_ARG, what
    assert check(far, 8, 8, sample_bytes=2, maxval=0, dst=False) == (0, "")   # (only a decode reads a maxval)
    # more windows than a call's launches have planes for: 65535 planes to encode, a third of that to decode
    many = [BASE + i * 64 for i in range(21846)]
    assert check(many[:21845], 8, 8)[0] == 0 and check(many[:21845], 8, 8, channels=3, dst=False)[0] == 0
    for dst, channels in ((True, 1), (False, 3)):
        rc, text = check(many, 8, 8, dst=dst, channels=channels)
        assert rc == ERR_ARG and ("21846" in text or "65538" in text), text


# ---- the list helper of the package ---------------------------------------------------------------------------------------

def test_view_list_fields_takes_one_shape_one_set_of_strides_and_one_dtype():
    import torch

    frame = torch.zeros((40, 64, 3), dtype=torch.uint8)
    boxes = [frame[2:12, 4:16], frame[20:30, 30:42], frame[2:12, 16:28]]
    f, ptrs = dwt_amd.view_list_fields(boxes)
    assert (f["W"], f["H"], f["channels"], f["n"], f["row_pitch"], f["channel_stride"], f["pixel_step"]) == (12, 10, 3, 3, 192, 0, 0)
    assert ptrs == [b.data_ptr() for b in boxes]
    chw = torch.zeros((3, 10, 12), dtype=torch.float16)
    f, _ = dwt_amd.view_list_fields([chw.permute(1, 2, 0)])
    assert (f["channel_stride"], f["row_pitch"], f["pixel_step"]) == (120, 12, 0)
    rgba = torch.zeros((10, 12, 4), dtype=torch.uint8)
    assert dwt_amd.view_list_fields([rgba[..., :3]], stepped=True)[0]["pixel_step"] == 4
    other = torch.zeros((10, 12, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="window 2 has strides"):
        dwt_amd.view_list_fields([boxes[0], boxes[1], other])
    with pytest.raises(ValueError, match="window 1 has shape"):
        dwt_amd.view_list_fields([boxes[0], frame[2:12, 4:20]])
    with pytest.raises(ValueError, match="window 1 has dtype"):
        dwt_amd.view_list_fields([other, other.to(torch.int16)])
    with pytest.raises(ValueError):
        dwt_amd.view_list_fields([])
    with pytest.raises(ValueError):
        dwt_amd.view_list_fields([frame[None, 2:12, 4:16]])
