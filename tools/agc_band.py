#!/usr/bin/env python3
"""The AGC tail against the tails it replaces, on the airband geometry: 760 channels of 25 kHz -> 8 kHz audio in a
20 MSPS buffer, AM and USB.  GPU box.

One Tuner, one loaded spectrum; per class two batched handles, AGC off and on.  The step is what run_all launches after
the load (rcfm_pipeline_run over all channels).  The four handles alternate, 50 steps each, in one process after one
load, and the whole series runs twice.  Pass 1 times the steps with device events (profiler off).  Pass 2 reads the tail's
stage of each handle: am_tail / ssb_tail is k_am_tail / k_ssb_tail with AGC off and k_agc_tail with AGC on (the AGC tail
is timed as the stage it replaces).  Both move 8 A bytes per channel.  Writes profiles/agc_band.json and prints it.

    python tools/agc_band.py [--steps 50] [--warmup 10] [--out profiles/agc_band.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402

N, B, A, C = 20_000_000, 25000, 8000, 760
TAIL = {"AM": "am_tail", "USB": "ssb_tail"}


def spread(v):
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return {"median": round(float(q[2]), 5), "iqr": [round(float(q[1]), 5), round(float(q[3]), 5)],
            "min": round(float(q[0]), 5), "max": round(float(q[4]), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agc_band.json"))
    a = ap.parse_args()
    lib = hip.lib()
    centres = workloads.channel_grid(C, B)
    tuner = rc.Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, B, rc.USB(B, A, cuda=True))
    tuner.request_bandwidth(float(N))
    x = workloads.wideband(N, tuner.input_frequency, centres, B, gain=0.05, stereo=False, deviation=0.2 * B)
    tuner.load(x)
    handle = tuner._ready()
    demods = {}
    for k in ("AM", "USB"):
        kind = getattr(hip, "RCFM_" + k)
        agc = rc.AGC(0.3, floor=1e-3)._settings(A, 1.0 if k == "AM" else 0.25)
        demods[k] = tuner._batched_demod(kind, B, A, 75e-6, 0)
        demods[k + "_agc"] = tuner._batched_demod(kind, B, A, 75e-6, 0, agc)
    audio = torch.empty((C, A, 1), dtype=torch.float32, device="cuda")
    s = hip.stream()

    def step(k):
        hip.check(lib.rcfm_pipeline_run(handle, demods[k], 0, C, hip.ptr(audio), s))

    out = {"config": {"N": N, "B": B, "A": A, "channels": C, "steps": a.steps, "warmup": a.warmup,
                      "step": "rcfm_pipeline_run over all channels after one tuner load",
                      "tail_bytes_per_launch": 8.0 * A * C}, "series": []}
    for series in range(2):
        for _ in range(a.warmup):
            for k in demods:
                step(k)
        torch.cuda.synchronize()
        ms = {k: [] for k in demods}
        for _ in range(a.steps):
            for k in demods:                 # alternating: every handle sees the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(k)
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        # the tail's stage, step by step, the handles alternating as above
        tail = {k: [] for k in demods}
        for _ in range(a.steps):
            for k in demods:
                st = TAIL[k.split("_")[0]]
                hip.check(lib.rcfm_profile_reset())
                hip.check(lib.rcfm_profile_enable(ctypes.c_uint64((1 << lib.rcfm_profile_stage_count()) - 1)))
                step(k)
                torch.cuda.synchronize()
                prof = bench.read_profile(lib)
                hip.check(lib.rcfm_profile_enable(ctypes.c_uint64(0)))
                assert prof[st][2] == 1, (k, prof[st])
                tail[k].append(prof[st][1] * 1e3)
        rec = {"step_ms": {k: spread(ms[k]) for k in demods}, "tail_us": {k: spread(tail[k]) for k in demods}}
        for k in ("AM", "USB"):
            rec["agc_tail_over_" + TAIL[k]] = round(rec["tail_us"][k + "_agc"]["median"] / rec["tail_us"][k]["median"], 3)
            rec["agc_step_over_step_" + k] = round(rec["step_ms"][k + "_agc"]["median"] / rec["step_ms"][k]["median"], 4)
        out["series"].append(rec)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
