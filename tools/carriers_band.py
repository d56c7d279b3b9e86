#!/usr/bin/env python3
"""Carrier estimates on the airband geometry: 760 channels of 25 kHz in a 20 MSPS buffer.  GPU box.

One AM Tuner, one loaded spectrum (the buffer of tools/squelch_band.py); two steps alternate in one process:
    carriers   rcfm_tuner_carriers over all channels, all four outputs (gate 0)
    levels     rcfm_tuner_levels over all channels -- the yardstick: the same 8 B bytes per channel, the same reduction shape
Each step is timed with device events (profiler off), `--steps` alternating rounds, the whole series `--series` times:
median and IQR per step and series, and the ratio of the medians.  Prints one JSON line.

    python tools/carriers_band.py [--steps 50] [--warmup 10] [--series 2]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402
from squelch_band import A, B, C, N, ON_AIR, band  # noqa: E402


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
    power = torch.empty(C, dtype=torch.float32, device="cuda")
    peak_bin = torch.empty(C, dtype=torch.int32, device="cuda")
    peak_power, centroid, spread = (torch.empty(C, dtype=torch.float32, device="cuda") for _ in range(3))
    s = hip.stream()

    def carriers():
        hip.check(lib.rcfm_tuner_carriers(handle, 0, C, ctypes.c_float(0.0), hip.ptr(peak_bin), hip.ptr(peak_power),
                                          hip.ptr(centroid), hip.ptr(spread), s))

    def levels():
        hip.check(lib.rcfm_tuner_levels(handle, 0, C, hip.ptr(power), s))

    steps = {"carriers": carriers, "levels": levels}
    for _ in range(a.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    pb = peak_bin.cpu().numpy()
    assert not pb[list(ON_AIR)].any(), "the stations of this buffer sit on their channel centres"

    def spread_of(v):
        q = np.percentile(v, [0, 25, 50, 75, 100])
        return {"median_ms": round(float(q[2]), 4), "iqr_ms": [round(float(q[1]), 4), round(float(q[3]), 4)],
                "min_ms": round(float(q[0]), 4), "max_ms": round(float(q[4]), 4)}

    out = {"config": {"N": N, "B": B, "channels": C, "on_air": len(ON_AIR), "steps": a.steps, "warmup": a.warmup,
                      "series": a.series, "algorithmic_bytes": 8.0 * B * C}, "series": []}
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
        block = {k: spread_of(v) for k, v in ms.items()}
        block["carriers_over_levels"] = round(block["carriers"]["median_ms"] / block["levels"]["median_ms"], 3)
        out["series"].append(block)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
