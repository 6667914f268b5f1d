#!/usr/bin/env python3
"""Generate tests/golden/refsweep.json with the REAL reference (oracle/_ref, built by oracle/Makefile target `ref`).

Runs _ref/encode and _ref/decode on the seeded cases of tests/refsweep.py and records what they did: per case the
input's sha256, per CAPACITY the stream's sha256, length and the three stderr lines, per decode the exit code and the
output's shape and sha256; per root-cut picture one [meta, root, total, KiB] row per CAPACITY; what the encoder does
with the four pictures that are too small; what the decoder does with PIXELS = -5.  Data only.  The file stays below
the size of smpte.pnm: cases that do not fit are dropped from the tail (tests/refsweep.py chunks() follows the record).
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orc  # noqa: E402
import refsweep  # noqa: E402

LIMIT = os.path.getsize(os.path.join(HERE, "smpte.pnm")) - 1024
NEG_PIXELS = 8


def line(obj):
    return json.dumps(obj, separators=(",", ":"))


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all", "ref"], check=True)
    assert orc.have_ref(), "needs the reference's sources to build oracle/_ref"
    with tempfile.TemporaryDirectory() as td:
        encode, decode = refsweep.ref_coder(td)
        refused = []
        for k, (W, H, Cn) in enumerate(refsweep.REFUSED):
            pix = refsweep.refused(k)
            assert encode(pix, 0) is None, "the reference takes a side below 8 after all?"
            refused.append([W, H, Cn, refsweep.sha(pix.tobytes()), 1])
        rootcut = [refsweep.rootcut_record(refsweep.RootCut(j), encode) for j in range(refsweep.ROOTCUT)]
        assert sum(r["C"] == 3 for r in rootcut) == 12 and {"impulses", "ramps"} <= {r["what"] for r in rootcut}
        neg = []
        for i in range(NEG_PIXELS):
            c = refsweep.Case(i)
            whole = encode(c.pix, 0)[0]
            neg.append([refsweep.decode_row(whole, decode(whole, px), c.W, c.H, c.C) for px in (-5, 0)])
        head = ['"seed":%d' % refsweep.SEED, '"refused":' + line(refused), '"neg_pixels":' + line(neg),
                '"rootcut":[\n' + ",\n".join(line(r) for r in rootcut) + "\n]"]
        size = sum(len(h) + 2 for h in head) + 32
        cases = []
        for i in range(refsweep.CASES):
            text = line(refsweep.case_record(refsweep.Case(i), encode, decode))   # no case is skipped
            if size + len(text) + 2 > LIMIT:
                break
            size += len(text) + 2
            cases.append(text)
            print(i, len(text), size, flush=True)
    # section 6 of the issue: caps, not measurements — another SEED if one breaks
    damaged = [d for c in map(json.loads, cases) for d in c["dec"][-6:] if len(c["dec"]) > 10]
    many = sum(len(d) == 5 for d in damaged)
    unreadable = sum(d[0] != 0 for d in damaged)
    assert many * 50 <= len(damaged), (many, len(damaged))
    assert unreadable * 20 <= len(damaged), (unreadable, len(damaged))
    out = "{\n" + ",\n".join(head + ['"cases":[\n' + ",\n".join(cases) + "\n]"]) + "\n}\n"
    assert len(out) < os.path.getsize(os.path.join(HERE, "smpte.pnm"))
    json.loads(out)
    open(refsweep.RECORD, "w").write(out)
    rec = json.loads(out)
    print(f"{len(cases)} cases, {sum(len(c['enc']) for c in rec['cases'])} streams, {sum(len(c['dec']) for c in rec['cases'])} decodes, "
          f"{len(damaged)} damaged ({many} claim more than 16 planes, {unreadable} unreadable), "
          f"{sum(len(r['rows']) for r in rootcut)} root-cut rows, {len(out)} bytes")


if __name__ == "__main__":
    main()
