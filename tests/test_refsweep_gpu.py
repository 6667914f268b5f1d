"""GPU: the library against tests/golden/refsweep.json — what the reference's own binaries did with the seeded cases
of tests/refsweep.py — directly, not through the oracle: stream bytes and the three statistics lines under three
capacities, decoded pictures of whole, cut and damaged streams with and without PIXELS, refusals, and the statistics
under every CAPACITY that cuts into header or root image."""
import os
import subprocess

import pytest

import orc
import refsweep

pytestmark = pytest.mark.gpu
REC = refsweep.record()
ENC = os.path.join(orc.ROOT, "bin", "encode")
DEC = os.path.join(orc.ROOT, "bin", "decode")


def lines_of(st):
    return refsweep.stat_lines(st.meta_bits, st.root_bits, st.total_bits, st.kib)


def same_picture(got, row):
    if row[0]:
        return got is None
    return got is not None and [got.shape[0], got.shape[1], refsweep.sha(got.tobytes())] == row[1:4]


@pytest.mark.parametrize("chunk", refsweep.chunks())
def test_library_against_the_record(ctx, chunk):
    for i in refsweep.chunk_cases(chunk):
        case, want = refsweep.Case(i), REC["cases"][i]
        where = (i, case.W, case.H, case.C)
        assert refsweep.sha(case.pix.tobytes()) == want["in"], ("the generator drifted", i)
        whole = None
        for cap, digest, length, lines in want["enc"]:
            data, st = ctx.encode(case.pix, cap)
            assert (len(data), refsweep.sha(data)) == (length, digest), (where, "capacity", cap)
            assert lines_of(st) == lines, (where, "capacity", cap)
            whole = data if whole is None else whole
        decs = case.decodes(whole, [e[0] for e in want["enc"]])
        assert len(decs) == len(want["dec"])
        batches = {}   # one batch per PIXELS value; the whole stream is the first of each (a batch takes its geometry from it)
        for k, (blob, px) in enumerate(decs):
            batches.setdefault(px, []).append(k)
        for px, ks in batches.items():
            assert decs[ks[0]][0] == whole
            outs = ctx.decode([decs[k][0] for k in ks], -1 if px is None else px)
            for k, got in zip(ks, outs):
                row = want["dec"][k]
                if len(row) == 5:   # claims more than 16 bit planes: the reference decodes on, the library says status 2
                    assert got is None and ctx.decode_planes([decs[k][0]], case.W, case.H, case.C)[1][0].status == 2, (where, "decode", k)
                else:
                    assert same_picture(got, row), (where, "decode", k, "PIXELS", px)


def test_pictures_with_a_side_below_8_are_refused(ctx):
    for k, (W, H, Cn, digest, code) in enumerate(REC["refused"]):
        pix = refsweep.refused(k)
        assert pix.shape == (H, W, Cn) and refsweep.sha(pix.tobytes()) == digest and code == 1
        with pytest.raises(RuntimeError):
            ctx.encode(pix)


@pytest.mark.parametrize("j", range(refsweep.ROOTCUT))
def test_statistics_under_every_capacity_that_cuts_into_header_or_root(ctx, j):
    """k_plan's count of what the reference's bit writer would say (pack.hip HdrWriter::rc_*), against the reference's
    own numbers: every CAPACITY from 1 to header + root image + 12 bytes."""
    rc, want = refsweep.RootCut(j), REC["rootcut"][j]
    assert refsweep.sha(rc.pix.tobytes()) == want["in"], ("the generator drifted", j)
    wrong = []
    for cap, row in enumerate(want["rows"], 1):
        st = ctx.encode(rc.pix, cap)[1]
        got = [st.meta_bits, st.root_bits, st.total_bits, st.kib]
        if got != row:
            wrong.append((cap, row, got))
    assert not wrong, (want["what"], rc.W, rc.H, rc.C, "capacity, reference, library", wrong[:8])


def test_cli_statistics_lines_on_root_cut_rows(tmp_path):
    """bin/encode prints the library's numbers in the reference's words: eight rows inside the root image of RGB pictures."""
    picked = [j for j in range(refsweep.ROOTCUT) if REC["rootcut"][j]["C"] == 3][:8]
    for n, j in enumerate(picked):
        rc, rows = refsweep.RootCut(j), REC["rootcut"][j]["rows"]
        cap = 7 + (n * 11) % max(1, len(rows) - 19)   # past the header, before the root image's end
        orc.write_pnm(str(tmp_path / "i.pnm"), rc.pix)
        r = subprocess.run([ENC, "i.pnm", "o.dwt", str(cap)], cwd=tmp_path, capture_output=True, timeout=120)
        assert r.returncode == 0
        assert r.stderr.decode().splitlines() == refsweep.stat_lines(*rows[cap - 1]), (j, cap)


def test_cli_negative_pixels_argument(ctx, tmp_path):
    """PIXELS = -5: the reference's decoder drops every level (decode.c:166-168), bin/decode clamps to 0 — same picture."""
    for i, (neg, zero) in enumerate(REC["neg_pixels"]):
        case = refsweep.Case(i)
        data = ctx.encode(case.pix)[0]
        assert refsweep.sha(data) == REC["cases"][i]["enc"][0][1]
        (tmp_path / "d.dwt").write_bytes(data)
        r = subprocess.run([DEC, "d.dwt", "d.pnm", "-5"], cwd=tmp_path, capture_output=True, timeout=120)
        assert r.returncode == neg[0] == 0
        assert same_picture(orc.read_pnm(str(tmp_path / "d.pnm")), neg), i
