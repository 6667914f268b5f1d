"""Seeded cases for the sweeps that pin the oracle and the library on the reference's own binaries.

One generator, three users: tests/golden/make_refsweep.py runs oracle/_ref on every case and writes
tests/golden/refsweep.json; tests/test_refsweep_cpu.py holds the oracle (and, where oracle/_ref is built, fresh
runs of the binaries) against that record; tests/test_refsweep_gpu.py holds the library against it, not through
the oracle.  Everything here follows from (SEED, case number) and from the bytes of the case's whole stream, which
every user checks against the record before it derives cuts and damaged copies from them."""
import hashlib
import json
import os
import subprocess

import numpy as np

import orc

SEED = 1018
CASES = 240
CHUNK = 20
ROOTCUT = 16
RECORD = os.path.join(orc.GOLDEN, "refsweep.json")
REFUSED = [(7, 40, 1), (40, 7, 3), (5, 5, 1), (300, 3, 3)]   # a side below 8: encode.c:145
KINDS = ("synthetic", "synthetic", "synthetic", "flat", "checkerboard", "noise", "impulses", "ramps", "bars")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def picture(rng, W, H, Cn, what=None):
    """One of nine kinds of uint8 picture [H, W, Cn]; `what` None draws the kind."""
    if what is None:
        what = int(rng.integers(0, 9))
    if what <= 2:
        return orc.synth(W, H, Cn, int(rng.integers(0, 1 << 30)), int(rng.integers(0, 2)))
    y, x = np.mgrid[0:H, 0:W]
    if what == 3:     # flat
        img = np.full((H, W, Cn), int(rng.integers(0, 256)))
    elif what == 4:   # checkerboard of two levels, period 1..8
        per = int(rng.integers(1, 9))
        a, b = int(rng.integers(0, 256)), int(rng.integers(0, 256))
        img = np.where((((x // per) + (y // per)) & 1)[..., None] == 0, a, b) * np.ones((1, 1, Cn), dtype=np.int64)
    elif what == 5:   # white noise over the full range
        img = rng.integers(0, 256, (H, W, Cn))
    elif what == 6:   # a few impulses on black
        img = np.zeros((H, W, Cn), dtype=np.int64)
        k = int(rng.integers(1, 30))
        img[rng.integers(0, H, k), rng.integers(0, W, k)] = rng.integers(1, 256, (k, Cn))
    elif what == 7:   # ramps
        img = ((x * int(rng.integers(1, 5)) + y * int(rng.integers(0, 5))) // int(rng.integers(1, 9)))[..., None] + np.arange(Cn) * 40
    else:             # bars with hard edges plus one noisy channel
        img = ((x * 8 // W) * 36)[..., None] + np.zeros((1, 1, Cn), dtype=np.int64)
        img[..., Cn - 1] += rng.integers(0, 3, (H, W))
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8).reshape(H, W, Cn))


def corrupted_blobs(good, n=40, seed=7):
    """Damaged copies of a stream, header intact: bit flips, garbage runs, junk tails (needs more than 80 bytes)."""
    rng = np.random.default_rng(seed)
    blobs = []
    for case in range(n):
        b = bytearray(good)
        kind = case % 4
        if kind == 0:
            for _ in range(int(rng.integers(1, 4))):
                i = int(rng.integers(6, len(b)))
                b[i] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            i = int(rng.integers(6, len(b) - 40))
            b[i:i + 32] = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        elif kind == 2:
            i = int(rng.integers(40, len(b)))
            b[i:] = bytes(rng.integers(0, 256, len(b) - i, dtype=np.uint8))
        else:
            i = int(rng.integers(40, len(b)))
            b[i:] = bytes([0 if case % 8 == 3 else 255]) * (len(b) - i)
        blobs.append(bytes(b))
    return blobs


def stat_lines(meta, root, total, kib):
    """encode.c:176,180,230"""
    return [f"{meta} bits for meta data", f"{root} bits for root image", f"{total} bits ({kib} KiB) encoded"]


def preamble_bytes(lines):
    """Bytes of header + root image, from the first two statistics lines of an encode without CAPACITY."""
    return (int(lines[0].split()[0]) + int(lines[1].split()[0]) + 7) // 8


def tiny_capacity_pictures():
    """Pictures for the tests of the statistics lines under tiny capacities: two synthetic ones and two RGB pictures of
    impulses on black, 211x51, whose root image line depends on the order a refused put_vli() leaves behind."""
    return [orc.synth(53, 37, 3, 4, 0), orc.synth(64, 40, 1, 9, 0)] + [picture(np.random.default_rng(s), 211, 51, 3, 6) for s in (18, 3)]


class Case:
    def __init__(self, i):
        self.i = i
        rng = np.random.default_rng([SEED, i])
        W, H = int(rng.integers(8, 401)), int(rng.integers(8, 401))
        shape = i % 5
        if shape == 0:      # power-of-two square
            W = H = int(2 ** rng.integers(3, 10))
        elif shape == 1:    # one short side: one or two levels on it
            if rng.integers(0, 2):
                W = int(rng.integers(8, 21))
            else:
                H = int(rng.integers(8, 21))
        elif shape == 2:    # the fused 8-bit kernels take widths that are a multiple of 4
            W = (W + 3) // 4 * 4
        elif shape == 3:    # a power of two +- 1 on one side or on both
            sides = [int(2 ** rng.integers(4, 9)) + (1 if rng.integers(0, 2) else -1) for _ in range(2)]
            pick = int(rng.integers(0, 3))
            W, H = (sides[0], H) if pick == 0 else (W, sides[1]) if pick == 1 else (sides[0], sides[1])
        self.W, self.H = W, H
        self.C = 1 if rng.integers(0, 2) else 3
        self.pix = picture(rng, W, H, self.C)

    def capacities(self, preamble):
        """CAPACITY values: none, one that cuts into header, root image or the first bytes after them, one further on."""
        rng = np.random.default_rng([SEED, self.i, 1])
        return [0, int(rng.integers(1, preamble + 13)), int(rng.integers(40, 3001))]

    def decodes(self, whole, caps):
        """[(blob, PIXELS or None)] from the whole stream: the whole stream under five PIXELS values (first, so that a
        batch of any one value starts with it), the capacity-cut streams, three cuts, six damaged copies."""
        rng = np.random.default_rng([SEED, self.i, 2])
        big, small = int(rng.integers(0, 3 * self.W * self.H + 2)), int(rng.integers(0, 200))
        out = [(whole, None), (whole, 0), (whole, 1), (whole, big), (whole, small)]
        out += [(whole[:c], None) for c in caps if c]   # a CAPACITY stream is that prefix (the record's hash says so)
        out += [(whole[:int(k)], None) for k in rng.integers(6, max(7, len(whole)), 3)]
        if len(whole) > 100:
            blobs = corrupted_blobs(whole, 6, int(rng.integers(0, 1 << 30)))
            out += [(b, big if j & 1 else None) for j, b in enumerate(blobs)]
        return out


class RootCut:
    """A picture coded under every CAPACITY from 1 to header + root image + 12 bytes."""
    WHAT = (6, 7, 5, 0, 6, 7, 8, 4, 6, 7, 3, 1, 6, 7, 5, 8)

    def __init__(self, j):
        rng = np.random.default_rng([SEED, j, 3])
        self.W, self.H = int(rng.integers(8, 301)), int(rng.integers(8, 301))
        self.C = 1 if j % 4 == 3 else 3
        self.what = KINDS[self.WHAT[j]]
        self.pix = picture(rng, self.W, self.H, self.C, self.WHAT[j])

    def capacities(self, preamble):
        return range(1, preamble + 13)


def refused(k):
    W, H, Cn = REFUSED[k]
    return picture(np.random.default_rng([SEED, k, 4]), W, H, Cn, 5)


# ---- the three coders behind one pair of calls: encode(pix, cap) -> (bytes, three lines) or None if refused,
# ---- decode(blob, PIXELS or None) -> picture or None

def ref_coder(tmp):
    tmp = str(tmp)

    def encode(pix, cap):
        orc.write_pnm(os.path.join(tmp, "i.pnm"), pix)
        r = subprocess.run([os.path.join(orc.REF_DIR, "encode"), "i.pnm", "o.dwt"] + ([str(cap)] if cap else []),
                           cwd=tmp, capture_output=True, timeout=120)
        if r.returncode:
            return None
        return open(os.path.join(tmp, "o.dwt"), "rb").read(), r.stderr.decode().splitlines()

    def decode(blob, px):
        open(os.path.join(tmp, "d.dwt"), "wb").write(blob)
        r = subprocess.run([os.path.join(orc.REF_DIR, "decode"), "d.dwt", "d.pnm"] + ([] if px is None else [str(px)]),
                           cwd=tmp, capture_output=True, timeout=120)
        return None if r.returncode else orc.read_pnm(os.path.join(tmp, "d.pnm"))

    return encode, decode


def orc_coder():
    def encode(pix, cap):
        try:
            data, st = orc.encode(pix, cap)
        except ValueError:
            return None
        return data, stat_lines(st.meta_bits, st.root_bits, st.total_bits, st.kib)

    return encode, lambda blob, px: orc.decode(blob, -1 if px is None else px)


def claims_many_planes(blob, W, H, Cn):
    """More than 16 bit planes claimed: only damage does that; the library refuses such a stream."""
    st = orc.decode_stage(blob, W, H, Cn, -1)
    return st is not None and max(st[3]) > 16


def decode_row(blob, back, W, H, Cn):
    """A decode in the record: [exit code, height, width, sha256] (+ "planes>16"), or [1, null] for a refused stream."""
    if back is None:
        return [1, None]
    return [0, back.shape[0], back.shape[1], sha(back.tobytes())] + (["planes>16"] if claims_many_planes(blob, W, H, Cn) else [])


def case_record(case, encode, decode):
    whole, lines = encode(case.pix, 0)
    caps = case.capacities(preamble_bytes(lines))
    enc = [[0, sha(whole), len(whole), lines]]
    for cap in caps[1:]:
        data, ln = encode(case.pix, cap)
        enc.append([cap, sha(data), len(data), ln])
    dec = [decode_row(blob, decode(blob, px), case.W, case.H, case.C) for blob, px in case.decodes(whole, caps)]
    return {"W": case.W, "H": case.H, "C": case.C, "in": sha(case.pix.tobytes()), "enc": enc, "dec": dec}


def rootcut_record(rc, encode):
    lines = encode(rc.pix, 0)[1]
    rows = []
    for cap in rc.capacities(preamble_bytes(lines)):
        ln = encode(rc.pix, cap)[1]
        rows.append([int(ln[0].split()[0]), int(ln[1].split()[0]), int(ln[2].split()[0]), int(ln[2].split("(")[1].split()[0])])
    return {"W": rc.W, "H": rc.H, "C": rc.C, "what": rc.what, "in": sha(rc.pix.tobytes()), "rows": rows}


_record = None


def record():
    global _record
    if _record is None:
        _record = json.load(open(RECORD))
    return _record


def chunks():
    """Numbers of the chunks of CHUNK cases the record holds (its tail may have been dropped for size)."""
    return list(range((len(record()["cases"]) + CHUNK - 1) // CHUNK))


def chunk_cases(k):
    return range(k * CHUNK, min((k + 1) * CHUNK, len(record()["cases"])))
