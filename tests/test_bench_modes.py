"""bench.py's two modes: a plain run only times the headline; --full adds every other measurement and check.

CPU: --full is an option, off by default.
GPU: on the `small` configuration, the blocks each mode carries -- one GPU, and two ranks as a gloo dry run on ONE
device (tests/test_bench_multirank.py runs the same launches with --full)."""

import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT, have_gpu

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

needs_gpu = pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")

# what only --full measures or checks at N = 1
FULL_ONLY = ("stages", "pipelined", "pcie_inclusive", "parity_vs_oracle", "other_configs", "surface")


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--full"])
    assert bench.parse_args().full is True


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _line(cmd, env=None, timeout=800):
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(r, steps, warmup):
    assert r["steps"] == steps and r["warmup"] == warmup and r["unit"] == "Msamples/s" and r["dtype"] == "f32"
    assert r["higher_is_better"] is True and r["metric"].startswith("IQ Msamples/s through Tuner+")
    assert abs(r["value"] - r["config"]["wideband_samples"] / (r["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * r["value"]
    assert r["roofline"]["launch_us"] > 0                # the dominant stage's event pairs inside the timed region


@pytest.mark.gpu
@needs_gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("full", [False, True])
def test_one_gpu_line_of_each_mode(full):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--config", "small"] + (["--full"] if full else [])
    r = _line(cmd)
    _check_headline(r, 2, 1)
    assert r["n_gpus"] == 1 and len(r["placement"]["ms_per_step_by_set"]) == 4
    if not full:
        assert [k for k in FULL_ONLY if k in r] == [] and r["cpu_baseline"] is None
        return
    assert r["stages"][r["roofline"]["stage"]]["ms"] > 0
    assert r["pipelined"]["lanes"] == 2 and r["pcie_inclusive"]["value"] > 0
    assert r["cpu_baseline"]["value"] > 0
    assert r["parity_vs_oracle"]["max_rel_err"] <= r["parity_vs_oracle"]["tol"]
    assert "other_configs" not in r                      # cfg4 only


@pytest.mark.gpu
@needs_gpu
@pytest.mark.timeout(900)
def test_plain_two_rank_line_still_picks_the_faster_verified_partitioning():
    """`python bench.py --gpus 2` without --full: both partitionings and their gather checks (they decide `value`),
    no one-rank leg, self check, host-fed loop or ring timing pass."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(RCFM_BENCH_DEVICE="0", RCFM_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = _line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
               "--config", "small"], env=env)
    _check_headline(r, 3, 1)
    pt = r["partitionings"]
    assert pt["verified"] == {"replicated": True, "rotating": True}
    fastest = max(pt["value"], key=pt["value"].get)
    assert pt["published"] == fastest and r["value"] == pt["value"][fastest]
    other = "rotating" if fastest == "replicated" else "replicated"
    assert r[other]["value"] == pt["value"][other] and "self_check" not in r[other]
    assert r["n1"] is None and r["speedup_vs_n1"] is None and "self_check" not in r
    assert "pcie_inclusive" not in r and "pcie_inclusive" not in r[other]
    for leg in (r, r[other]):
        assert leg["gather_check"]["finite"] and leg["gather_check"]["blocks_with_audio"] == 2
    rot = r if fastest == "rotating" else r[other]
    for row in rot["per_rank"]:
        assert row["step_ms"] > 0 and row["send_ms"] is None and row["wait_ms"] is None and "owned_buffers" not in row
