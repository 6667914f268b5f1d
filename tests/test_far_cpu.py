"""CPU: the layouts of tests/far.py are what tests/test_far_gpu.py needs them to be.  Host arithmetic only: where the
rows of every case lie, what the library asks of a view, and where a product formed in 32 bits would land."""
import pytest

import far
from far import T31, T32

cases = pytest.mark.parametrize("case", far.CASES, ids=lambda c: c.name)


@cases
def test_the_claimed_offsets_are_there(case):
    """Some row of the case starts where each claim says: between 2^31 and 2^32 samples from the view's origin, beyond
    2^32 samples — or, for the 16-bit stack, where only the byte offset has passed the power of two."""
    starts = [sum(t) for t, _ in case.pieces()]
    assert min(starts) == 0
    for s_lo, s_hi, b_lo, b_hi in case.claims:
        assert any(s_lo <= s < s_hi and b_lo <= s * case.sb < b_hi for s in starts), (s_lo, s_hi, b_lo, b_hi)
    if case.below:
        assert max(starts) < case.below
    # far strides are a power of two plus a multiple of 4 that is no power of two
    assert far.D % 4 == 0 and far.D & (far.D - 1)
    big = [s for s in case.L.strides if s >= 1 << 26]
    assert big and all((s - (1 << (s.bit_length() - 1))) // far.D in (1, 3) or s - (1 << 26) in (12, 13) for s in big), big


@cases
def test_the_rows_lie_in_the_frame_and_apart(case):
    rows = far.true_rows(case)
    assert rows[0][0] >= far.HEAD * case.sb and rows[-1][1] <= case.frame_bytes
    assert all(a[1] <= b[0] for a, b in zip(rows, rows[1:])), "two rows of the case overlap"
    assert case.frame_bytes > T32


@cases
def test_wide_shapes_meet_the_wide_kernels_conditions_and_the_others_do_not(case):
    assert far.wide_conditions(case) == case.wide
    if not case.wide:   # W = 131, an origin off the quad grid, or a step the wide kernels do not take
        assert case.W % 4 or case.L.off % 4 or (case.step and case.Cn == 1)
    assert case.L.strides[-3] < T31, "the row pitch must fit the kernels' int"


@cases
def test_no_case_is_refused_for_overlapping_windows(case):
    assert far.decode_view_accepts(case) is None


@cases
def test_a_product_formed_in_32_bits_lands_in_the_frame_and_on_no_window(case):
    """Every wrong place: inside the allocation (no fault) and on frame that holds the fill value (the bytes differ)."""
    rows = far.true_rows(case)
    stray = far.stray_rows(case)
    assert stray, "nothing in this case exceeds 32 bits"
    for a, b, what in stray:
        assert 0 <= a and b <= case.frame_bytes, (what, a, b)
        assert not far.overlaps(rows, a, b), (what, a, b)
    kinds = {what.split(" as ")[1] for _, _, what in stray}
    want = {"int samples", "unsigned samples", "int bytes", "unsigned bytes"}
    assert want - ({"unsigned samples"} if case.below else set()) <= kinds   # (below: no sample offset reaches 2^32, on purpose)


def test_the_switched_cases_have_enough_windows_for_parts():
    for name in far.SWITCHED:
        assert far.BY_NAME[name].L.n >= 4   # fewer than four images are one part (unpack.hip)
    assert {far.BY_NAME[n].wide for n in far.SWITCHED} == {True, False}


def test_every_kind_of_layout_has_a_wide_and_a_general_case_and_every_depth_and_colour_occurs():
    assert {(c.Cn, c.is16) for c in far.CASES} == {(1, False), (3, False), (1, True), (3, True)}
    for kind in ("stack", "grid", "planar-cs", "planar-img", "rgbx8", "far-row"):
        assert {c.wide for c in far.CASES if c.name.startswith(kind)} == {True, False}, kind
