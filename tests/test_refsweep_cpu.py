"""CPU: the oracle against tests/golden/refsweep.json, the record the reference's own binaries left of the seeded
cases of tests/refsweep.py (bytes, statistics lines, decoded pictures, refusals) — and, where oracle/_ref is built,
the record against fresh runs of those binaries, so that it cannot rot."""
import pytest

import orc
import refsweep

REC = refsweep.record()


def test_the_record_is_this_generators():
    assert REC["seed"] == refsweep.SEED
    assert 0 < len(REC["cases"]) <= refsweep.CASES and len(REC["rootcut"]) == refsweep.ROOTCUT


@pytest.mark.parametrize("chunk", refsweep.chunks())
def test_oracle_against_the_record(chunk, tmp_path):
    coders = [("oracle", refsweep.orc_coder())] + ([("oracle/_ref", refsweep.ref_coder(tmp_path))] if orc.have_ref() else [])
    for i in refsweep.chunk_cases(chunk):
        case = refsweep.Case(i)
        want = REC["cases"][i]
        assert refsweep.sha(case.pix.tobytes()) == want["in"], ("the generator drifted", i)
        for who, (encode, decode) in coders:
            got = refsweep.case_record(case, encode, decode)
            assert got["enc"] == want["enc"], (who, i, case.W, case.H, case.C)
            for k, (g, w) in enumerate(zip(got["dec"], want["dec"])):
                assert g == w, (who, i, case.W, case.H, case.C, "decode", k)
            assert len(got["dec"]) == len(want["dec"])


def test_pictures_with_a_side_below_8_are_refused(tmp_path):
    for k, (W, H, Cn, digest, code) in enumerate(REC["refused"]):
        pix = refsweep.refused(k)
        assert pix.shape == (H, W, Cn) and refsweep.sha(pix.tobytes()) == digest and code == 1
        with pytest.raises(ValueError):
            orc.encode(pix)
        if orc.have_ref():
            assert refsweep.ref_coder(tmp_path)[0](pix, 0) is None


def test_negative_pixels_argument_is_pixels_0():
    """decode.c:166-168 compares every level's pixel count with atoi(PIXELS): a negative value drops all of them, like 0."""
    for i, (neg, zero) in enumerate(REC["neg_pixels"]):
        assert neg == zero and neg[0] == 0
        case = refsweep.Case(i)
        back = orc.decode(orc.encode(case.pix)[0], 0)
        assert [0, back.shape[0], back.shape[1], refsweep.sha(back.tobytes())] == neg


def test_statistics_under_every_capacity_that_cuts_into_header_or_root(tmp_path):
    """The root-cut list: every CAPACITY from 1 to header + root image + 12 bytes.  A refused byte ends the field that
    is being written, and a put_vli() ended part-way leaves its order raised (vli.h:70-80): the root image line of an
    RGB picture depends on that, because the next channel's bit count is coded from the order that was left."""
    coders = [("oracle", refsweep.orc_coder())] + ([("oracle/_ref", refsweep.ref_coder(tmp_path))] if orc.have_ref() else [])
    for j, want in enumerate(REC["rootcut"]):
        rc = refsweep.RootCut(j)
        assert refsweep.sha(rc.pix.tobytes()) == want["in"], ("the generator drifted", j)
        for who, (encode, _) in coders:
            got = refsweep.rootcut_record(rc, encode)
            wrong = [(cap + 1, w, g) for cap, (g, w) in enumerate(zip(got["rows"], want["rows"])) if g != w]
            assert not wrong and len(got["rows"]) == len(want["rows"]), (who, j, want["what"], rc.W, rc.H, rc.C, "capacity, reference, got", wrong[:8])
