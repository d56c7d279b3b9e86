#!/usr/bin/env python3
"""The wideband power spectrum on the airband geometry: a 20 MSPS buffer, 760 channels of 25 kHz.  GPU box.

One Tuner, one loaded spectrum (a dozen stations, the other channels empty); three steps alternate in one process:
    spectrum_wide    rcfm_tuner_power_spectrum, full span, 1600 cells of 12 500 bins (power and peak): reads 8 N bytes
    spectrum_narrow  the same with one bin per cell (cells = N): reads 8 N bytes, writes 2 x 4 N
    levels           rcfm_tuner_levels over the 760 channels: reads 8 B C bytes -- the yardstick, a one-pass float64
                     reduction over the same resident spectrum with 16-byte loads
Each step is timed with device events, `--steps` alternating rounds, the whole series `--series` times: median and IQR
per step and series, the bytes each step moves per second, and the spectrum steps' rate as a fraction of the levels
step's rate in the same series.  Prints one JSON line.

    python tools/spectrum_band.py [--steps 50] [--warmup 10] [--series 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402
from squelch_band import B, C, N, band  # noqa: E402

CELLS_WIDE = 1600


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
        tuner.add_channel(f, B, None)
    tuner.request_bandwidth(float(N))
    tuner.load(band(tuner.input_frequency, centres))
    handle = tuner._ready()
    s = hip.stream()
    level = torch.empty(C, dtype=torch.float32, device="cuda")
    wide = [torch.empty(CELLS_WIDE, dtype=torch.float32, device="cuda") for _ in range(2)]
    narrow = [torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(2)]

    def spectrum_wide():
        hip.check(lib.rcfm_tuner_power_spectrum(handle, -(N // 2), N, CELLS_WIDE, hip.ptr(wide[0]), hip.ptr(wide[1]), s))

    def spectrum_narrow():
        hip.check(lib.rcfm_tuner_power_spectrum(handle, -(N // 2), N, N, hip.ptr(narrow[0]), hip.ptr(narrow[1]), s))

    def levels():
        hip.check(lib.rcfm_tuner_levels(handle, 0, C, hip.ptr(level), s))

    steps = {"spectrum_wide": spectrum_wide, "spectrum_narrow": spectrum_narrow, "levels": levels}
    moved = {"spectrum_wide": 8.0 * N + 8.0 * CELLS_WIDE, "spectrum_narrow": 8.0 * N + 8.0 * N, "levels": 8.0 * B * C + 4.0 * C}
    for _ in range(a.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    total = float(wide[0].double().sum())
    assert abs(total - float(narrow[0].double().sum())) <= 1e-5 * total, "the two forms disagree on the band's power"

    def spread(v):
        q = np.percentile(v, [0, 25, 50, 75, 100])
        return {"median_ms": round(float(q[2]), 4), "iqr_ms": [round(float(q[1]), 4), round(float(q[3]), 4)],
                "min_ms": round(float(q[0]), 4), "max_ms": round(float(q[4]), 4)}

    out = {"config": {"N": N, "B": B, "channels": C, "cells_wide": CELLS_WIDE, "cells_narrow": N, "steps": a.steps,
                      "warmup": a.warmup, "series": a.series, "bytes_moved": moved}, "series": []}
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
        for k in steps:
            block[k]["TBps"] = round(moved[k] / (block[k]["median_ms"] * 1e-3) / 1e12, 3)
        for k in ("spectrum_wide", "spectrum_narrow"):
            block[k]["rate_vs_levels"] = round(block[k]["TBps"] / block["levels"]["TBps"], 3)
        out["series"].append(block)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
