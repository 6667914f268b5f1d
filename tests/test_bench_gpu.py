"""`python bench.py --gpus 1` on an MI355X: a plain run prints the headline only, and --dump-outputs writes what the
last timed step computed — the same from run to run, and equal to the oracle's streams and to the input pixels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import orc

pytestmark = pytest.mark.gpu

NAMES = ("stream_lengths.npy", "decoded_pixels.npy", "stream_bytes.npy")


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    W, H, C, frames = 256, 192, 3, 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    dumps = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(orc.ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--frames", str(frames), "--geometry", str(W), str(H), str(C), "--dump-outputs", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["bit_exact"]["roundtrip_lossless"] is True
        assert not {"roofline", "roofline_codec", "coder", "cpu_baseline", "workloads"} & set(line)
        dumps.append({n: np.load(out / n) for n in NAMES})

    for n in NAMES:
        assert dumps[0][n].dtype in (np.float32, np.float64)
        assert np.array_equal(dumps[0][n], dumps[1][n]), n
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20

    got = dumps[0]
    want = [orc.encode(orc.synth(W, H, C, i, 0))[0] for i in range(frames)]    # bench.py: seed0 = rank * frames
    assert got["stream_lengths.npy"].tolist() == [len(w) for w in want]
    pix = np.concatenate([orc.synth(W, H, C, i, 0).ravel() for i in range(frames)])
    assert np.array_equal(got["decoded_pixels.npy"], pix.astype(np.float32))   # few enough pixels: all of them
    per_stream = max(min(bench.DUMP_STREAM_BYTES // frames, max(len(w) for w in want)), 1)
    frac = np.sort(np.random.default_rng(bench.DUMP_SEED).random(per_stream))
    for i, w in enumerate(want):
        pos = np.minimum((frac * len(w)).astype(np.int64), len(w) - 1)
        assert np.array_equal(got["stream_bytes.npy"][i], np.frombuffer(w, dtype=np.uint8)[pos].astype(np.float32)), i
