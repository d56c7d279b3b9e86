#!/usr/bin/env python3
"""Signal levels and squelch on the airband geometry: 760 channels of 25 kHz -> 8 kHz audio in a 20 MSPS buffer.  GPU box.

One AM Tuner, one loaded spectrum (a dozen stations, the other channels empty); three steps alternate in one process:
    levels           Tuner.levels' launches alone (rcfm_tuner_levels over all channels)
    run_all          rcfm_pipeline_run over all channels, squelch off
    run_all_squelch  the same followed by rcfm_tuner_levels + rcfm_squelch on the stream, as Tuner.run_all queues them
Each step is timed with device events (profiler off), `--steps` alternating rounds, the whole series `--series` times:
median and IQR per step and series.  A last pass reads the stage profile and prices the two stages: levels reads 8 B
bytes per channel, squelch writes 4 A bytes per closed channel.  Prints one JSON line.

    python tools/squelch_band.py [--steps 50] [--warmup 10] [--series 2]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402
from radiocore.tools import squelch  # noqa: E402

N, B, A, C = 20_000_000, 25000, 8000, 760
HBM_PEAK = 8e12
ON_AIR = (80, 131, 200, 201, 333, 380, 415, 502, 590, 644, 645, 679)


def band(f_in, centres):
    """complex64 [N]: an AM carrier with one tone on each channel of ON_AIR, receiver noise everywhere."""
    X = np.zeros(N, np.complex128)
    t = np.arange(B) / B
    kk = np.fft.fftfreq(B, 1.0 / B).astype(np.int64)
    for j, i in enumerate(ON_AIR):
        s = 10.0 ** (-j / 11.0) * (1 + 0.5 * np.sin(2 * np.pi * (400.0 + 90.0 * j) * t))
        X[(kk + int(centres[i] - f_in)) % N] += np.fft.fft(s) * (N / B)
    x = np.fft.ifft(X)
    rng = np.random.default_rng(5)
    x += 1e-4 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return x.astype(np.complex64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--series", type=int, default=2)
    a = ap.parse_args()
    lib = hip.lib()
    centres = workloads.channel_grid(C, B)
    tuner = rc.Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, B, rc.AM(B, A, cuda=True))
    tuner.request_bandwidth(float(N))
    tuner.load(band(tuner.input_frequency, centres))
    handle = tuner._ready()
    demod = tuner._batched_demod(hip.RCFM_AM, B, A, 75e-6, 0)
    thr = hip.to_device(squelch.threshold_over_floor(tuner.levels(), B, 10.0), torch.float32)
    audio = torch.empty((C, A, 1), dtype=torch.float32, device="cuda")
    power = torch.empty(C, dtype=torch.float32, device="cuda")
    mask = torch.empty(C, dtype=torch.uint8, device="cuda")
    s = hip.stream()

    def levels():
        hip.check(lib.rcfm_tuner_levels(handle, 0, C, hip.ptr(power), s))

    def run_all():
        hip.check(lib.rcfm_pipeline_run(handle, demod, 0, C, hip.ptr(audio), s))

    def run_all_squelch():
        run_all()
        levels()
        hip.check(lib.rcfm_squelch(hip.ptr(power), hip.ptr(thr), C, A, hip.ptr(audio), hip.ptr(mask), s))

    steps = {"levels": levels, "run_all": run_all, "run_all_squelch": run_all_squelch}
    for _ in range(a.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    opened = [int(i) for i in np.flatnonzero(mask.cpu().numpy())]
    closed = C - len(opened)

    def spread(v):
        q = np.percentile(v, [0, 25, 50, 75, 100])
        return {"median_ms": round(float(q[2]), 4), "iqr_ms": [round(float(q[1]), 4), round(float(q[3]), 4)],
                "min_ms": round(float(q[0]), 4), "max_ms": round(float(q[4]), 4)}

    out = {"config": {"N": N, "B": B, "A": A, "channels": C, "on_air": len(ON_AIR), "open": opened, "steps": a.steps,
                      "warmup": a.warmup, "series": a.series}, "series": []}
    assert opened == sorted(ON_AIR), opened
    for _ in range(a.series):
        ms = {k: [] for k in steps}
        for _ in range(a.steps):
            for k, fn in steps.items():              # alternating: every step sees the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        block = {k: spread(v) for k, v in ms.items()}
        block["squelch_cost_ms"] = round(block["run_all_squelch"]["median_ms"] - block["run_all"]["median_ms"], 4)
        out["series"].append(block)

    # the stage profile, on its own (events on the stream slow the steps down)
    reps = 20
    hip.check(lib.rcfm_profile_reset())
    hip.check(lib.rcfm_profile_enable(ctypes.c_uint64((1 << lib.rcfm_profile_stage_count()) - 1)))
    for _ in range(reps):
        run_all_squelch()
    torch.cuda.synchronize()
    prof = bench.read_profile(lib)
    hip.check(lib.rcfm_profile_enable(ctypes.c_uint64(0)))
    by = {"levels": 8.0 * B * C, "squelch": 4.0 * A * closed}
    out["stages"] = {}
    for name, (_, t_ms, cnt) in prof.items():
        if cnt == 0:
            continue
        t = t_ms / reps
        row = {"ms": round(t, 4), "launches": cnt / reps}
        if name in by:
            row.update({"algorithmic_bytes": by[name], "TBps": round(by[name] / (t * 1e-3) / 1e12, 3),
                        "frac_of_hbm_peak": round(by[name] / (t * 1e-3) / HBM_PEAK, 3)})
        out["stages"][name] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
