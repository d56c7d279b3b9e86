"""bench.py --dump-outputs: what the timed path computed in its last step, for output-for-output comparison of builds.

CPU: the seeded channel sample of a block too large to write whole.
GPU: the dump of a one-GPU run holds the audio of every channel of the `small` configuration, and two runs with
different handle-set layouts write the same audio bit for bit.  The dumped set has seen the same number of buffers in
both runs: bench.py runs its untimed profile step on set 0 only, so the one-set run (set 0: warm-up 1 + profile 1 +
3 timed) and the two-set run (set 1: warm-up 2 + 3 timed) each dump the fifth buffer through the de-emphasis state."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, have_gpu

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_sample_keeps_a_seeded_subset_of_a_large_block():
    C, A, ch = 1024, 48000, 2                                            # cfg4's audio block: 393 MB
    audio = torch.arange(C, dtype=torch.float32)[:, None, None].expand(C, A, ch)     # row i holds i
    d = bench.dump_sample(audio)
    rows = d["audio_channels"]
    assert d["audio"].dtype == np.float32 and rows.dtype == np.float64
    assert d["audio"].nbytes + rows.nbytes <= 64e6 and d["audio"].nbytes > bench.DUMP_BYTES - A * ch * 4
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < C
    assert np.array_equal(d["audio"][:, 0, 0], rows.astype(np.float32))
    assert np.array_equal(bench.dump_sample(audio)["audio_channels"], rows)      # the same sample every time
    small = bench.dump_sample(audio[:16])
    assert np.array_equal(small["audio_channels"], np.arange(16)) and small["audio"].shape == (16, A, ch)


def _bench_dump(out_dir, sets, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", str(warmup),
           "--config", "small", "--cpu-channels", "0", "--no-extras", "--no-pcie", "--placement-sets", str(sets),
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), np.load(out_dir / "audio.npy"), np.load(out_dir / "audio_channels.npy")


@pytest.mark.gpu
@pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")
@pytest.mark.timeout(1300)
def test_dump_outputs_of_a_one_gpu_run(tmp_path):
    N, C, B, A, _raster, kind = bench.CONFIGS["small"]
    r, audio, rows = _bench_dump(tmp_path / "one_set", 1, warmup=1)
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert abs(r["value"] - N / (r["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * r["value"]
    assert audio.dtype == np.float32 and audio.shape == (C, A, 2 if kind == "WBFM" else 1)
    assert rows.dtype == np.float64 and np.array_equal(rows, np.arange(C))
    assert np.all(np.isfinite(audio)) and np.all(np.abs(audio).max(axis=(1, 2)) > 1e-3)
    _, again, _ = _bench_dump(tmp_path / "two_sets", 2, warmup=2)
    assert np.array_equal(audio, again)
