"""GPU: `encode` with DWTX_WRITE_INDEX leaves the sidecar index its encoder wrote (dwtx_ctx_set_encode_index) beside the
stream: the very file `decode` with DWTX_WRITE_INDEX writes for that stream, and a later decode that finds it gives the
same picture."""
import os
import subprocess

import pytest

import orc

pytestmark = pytest.mark.gpu
ENC = os.path.join(orc.ROOT, "bin", "encode")
DEC = os.path.join(orc.ROOT, "bin", "decode")
SMPTE = os.path.join(orc.GOLDEN, "smpte.pnm")


def _run(cmd, **env):
    return subprocess.run(cmd, capture_output=True, timeout=300, env=dict(os.environ, **env))


@pytest.mark.parametrize("name", ["smpte", "gray_96x64", "rgb_53x37"])
def test_encode_leaves_the_index_decode_would_write(tmp_path, name):
    if name == "smpte":
        src = SMPTE
    else:
        src = str(tmp_path / "in.pnm")
        orc.write_pnm(src, orc.synth(96, 64, 1, 3, 0) if name == "gray_96x64" else orc.synth(53, 37, 3, 4, 1))
    pix = orc.read_pnm(src)
    dwt, pnm = str(tmp_path / "a.dwt"), str(tmp_path / "a.pnm")
    r = _run([ENC, src, dwt], DWTX_WRITE_INDEX="1")
    assert r.returncode == 0, r.stderr[-300:]
    assert open(dwt, "rb").read() == orc.encode(pix)[0]
    mine = open(dwt + ".idx", "rb").read()
    assert mine[:4] == b"DWTI" and len(mine) == 32 + 32 * int.from_bytes(mine[16:20], "little") > 32
    # the decoder's own index of the same stream, made without one to find
    dwt2 = str(tmp_path / "b.dwt")
    open(dwt2, "wb").write(open(dwt, "rb").read())
    r = _run([DEC, dwt2, pnm], DWTX_WRITE_INDEX="1")
    assert r.returncode == 0, r.stderr[-300:]
    assert open(dwt2 + ".idx", "rb").read() == mine
    # a later decode finds the encoder's file; a rejected index would be an error here
    os.remove(pnm)
    r = _run([DEC, dwt, pnm], DWTX_NO_INDEX_FALLBACK="1")
    assert r.returncode == 0, r.stderr[-300:]
    back = orc.read_pnm(pnm)
    assert back.shape == pix.shape and (back == pix).all()


def test_encode_asks_its_encoder_for_the_index_and_decodes_nothing():
    """The re-decode of the stream just written is gone: `encode` binds the encoder's call and no decode entry point."""
    blob = open(ENC, "rb").read()
    assert b"dwtx_ctx_set_encode_index" in blob
    assert b"dwtx_decode_images" not in blob and b"dwtx_ctx_set_index" not in blob
