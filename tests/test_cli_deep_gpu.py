"""GPU: bin/encode under DWTX_DEEP and bin/decode under DWTX_MAXVAL — deep PNM files (maxval 256..65535, two bytes per
sample, most significant first) — against tests/deep.py; without the variables both behave as before."""
import os
import subprocess

import numpy as np
import pytest

import deep
import orc

pytestmark = pytest.mark.gpu
ENC = os.path.join(orc.ROOT, "bin", "encode")
DEC = os.path.join(orc.ROOT, "bin", "decode")
REFUSAL = "only 8 bit per channel SRGB supported at the moment."


def run(*cmd, env=None, stdin=None):
    e = {k: v for k, v in os.environ.items() if k not in ("DWTX_DEEP", "DWTX_MAXVAL")}
    e.update(env or {})
    return subprocess.run(list(cmd), input=stdin, capture_output=True, timeout=300, env=e)


def pnm16(pix, maxval):
    H, W, Cn = pix.shape
    return b"P%d %d %d %d\n" % (5 if Cn == 1 else 6, W, H, maxval) + pix.astype(">u2").tobytes()


def read_pnm16(b, maxval):
    head, rest = b.split(b"\n", 1)
    magic, W, H, M = head.split()
    assert int(M) == maxval
    Cn = 1 if magic == b"P5" else 3
    assert len(rest) == 2 * int(W) * int(H) * Cn
    return np.frombuffer(rest, dtype=">u2").reshape(int(H), int(W), Cn).astype(np.uint16)


CASES = [("gray", lambda: deep.smooth_noise(256, 200, 1, 4095, 1), 4095), ("rgb", lambda: deep.noise(131, 77, 3, 4095, 2), 4095),
         ("rgb16", lambda: deep.smooth_noise(200, 120, 3, 65535, 3), 65535)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_deep_files_round_trip_and_equal_the_composed_oracle(tmp_path, case):
    _, make, M = case
    pix = make()
    H, W, Cn = pix.shape
    src, dwt, pnm = str(tmp_path / "i.pnm"), str(tmp_path / "a.dwt"), str(tmp_path / "o.pnm")
    open(src, "wb").write(pnm16(pix, M))
    want, st = deep.deep_encode(pix)
    r = run(ENC, src, dwt, env={"DWTX_DEEP": "1"})
    assert r.returncode == 0, r.stderr
    assert open(dwt, "rb").read() == want
    assert r.stderr.decode().splitlines() == [f"{st.meta_bits} bits for meta data", f"{st.root_bits} bits for root image",
                                              f"{st.total_bits} bits ({(len(want) + 512) // 1024} KiB) encoded"]
    r = run(DEC, dwt, pnm, env={"DWTX_MAXVAL": str(M)})
    assert r.returncode == 0, r.stderr
    assert open(pnm, "rb").read() == open(src, "rb").read()
    # CAPACITY, PIXELS and a truncated file
    cap = len(want) // 3
    assert run(ENC, src, dwt, str(cap), env={"DWTX_DEEP": "1"}).returncode == 0
    cut = open(dwt, "rb").read()
    assert cut == deep.deep_encode(pix, cap)[0] and cut == want[:cap]
    assert run(DEC, dwt, pnm, env={"DWTX_MAXVAL": str(M)}).returncode == 0
    assert (read_pnm16(open(pnm, "rb").read(), M) == deep.deep_decode(cut, W, H, Cn, M)).all()
    open(dwt, "wb").write(want)
    for px in (0, 3000):
        assert run(DEC, dwt, pnm, str(px), env={"DWTX_MAXVAL": str(M)}).returncode == 0
        ref = deep.deep_decode(want, W, H, Cn, M, px)
        got = read_pnm16(open(pnm, "rb").read(), M)
        assert got.shape == ref.shape and (got == ref).all()
    # pipes
    r = run(ENC, "-", "-", env={"DWTX_DEEP": "1"}, stdin=pnm16(pix, M))
    assert r.returncode == 0 and r.stdout == want
    r = run(DEC, "-", "-", env={"DWTX_MAXVAL": str(M)}, stdin=want)
    assert r.returncode == 0 and r.stdout == pnm16(pix, M)


def test_without_the_variables_both_behave_as_before(tmp_path):
    pix = deep.smooth_noise(64, 48, 3, 4095, 1)
    src, dwt, pnm = str(tmp_path / "i.pnm"), str(tmp_path / "a.dwt"), str(tmp_path / "o.pnm")
    open(src, "wb").write(pnm16(pix, 4095))
    r = run(ENC, src, dwt)
    assert r.returncode == 1 and REFUSAL in r.stderr.decode() and not os.path.exists(dwt)
    # a maxval below 255 stays refused with the switch too; an 8-bit file goes the 8-bit way under it
    low = str(tmp_path / "low.pnm")
    open(low, "wb").write(b"P5 64 48 100\n" + bytes(64 * 48))
    for env in (None, {"DWTX_DEEP": "1"}):
        r = run(ENC, low, dwt, env=env)
        assert r.returncode == 1 and REFUSAL in r.stderr.decode()
    p8 = orc.synth(64, 48, 3, 1, 0)
    orc.write_pnm(src, p8)
    assert run(ENC, src, dwt, env={"DWTX_DEEP": "1"}).returncode == 0
    assert open(dwt, "rb").read() == orc.encode(p8)[0]
    # decode without DWTX_MAXVAL writes an 8-bit file, clamped at 255 as ever
    data = deep.deep_encode(pix)[0]
    open(dwt, "wb").write(data)
    assert run(DEC, dwt, pnm).returncode == 0
    out = open(pnm, "rb").read()
    assert out.startswith(b"P6 64 48 255\n") and (orc.read_pnm(pnm) == deep.deep_decode(data, 64, 48, 3, 255)).all()
    for bad in ("0", "255", "65536", "x"):
        assert run(DEC, dwt, pnm, env={"DWTX_MAXVAL": bad}).returncode == 1


def test_decode_without_maxval_clamps_a_15_plane_stream_at_255(tmp_path):
    """The documented use at a size where it matters: 132x72 RGB takes the fused inverse kernel and the 16-bit ring planes,
    the stream's coefficients reach 32767 and the clamps cut about half of the samples (tests/test_deep_cpu.py)."""
    W, H, Cn = 132, 72, 3
    data = deep.foreign_stream(W, H, Cn, 15)[0]
    dwt, pnm = str(tmp_path / "a.dwt"), str(tmp_path / "o.pnm")
    open(dwt, "wb").write(data)
    r = run(DEC, dwt, pnm)
    assert r.returncode == 0, r.stderr
    assert open(pnm, "rb").read().startswith(b"P6 132 72 255\n") and (orc.read_pnm(pnm) == orc.decode(data)).all()


def test_a_picture_with_too_many_planes_is_refused(tmp_path):
    src, dwt = str(tmp_path / "i.pnm"), str(tmp_path / "a.dwt")
    open(src, "wb").write(pnm16(deep.noise(128, 96, 3, 65535, 1), 65535))
    r = run(ENC, src, dwt, env={"DWTX_DEEP": "1"})
    assert r.returncode == 1 and "needs more than 16 bit planes" in r.stderr.decode()
