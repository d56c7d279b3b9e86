#!/usr/bin/env python3
"""What the noise floor costs: rcfm_floor_run against a device copy and against the power spectrum it follows, and the airband
step with fixed squelch thresholds against OverFloor.  GPU box.

Alternating, `--rounds` blocks of `--steps` timed steps each, a step being `calls_per_step` calls back to back between two
device events (one call where a call takes milliseconds):
    floor_run       rcfm_floor_run at (M = 3200, half = 64), (M = 24 000, half = 128) and (M = 2^20, half = 512), guard 4,
                    lower quartile, floor and over both written
    memcpy_d2d      rcfm_memcpy_d2d of the same 4 M bytes: the device-copy yardstick
    power_spectrum  rcfm_tuner_power_spectrum of a loaded buffer into M cells (N = 2e7 for the first two, 2^22 bins for
                    M = 2^20): the call the floor follows
    thresholds      rcfm_floor_thresholds for 760 channels
and load + run_all of the 760-channel AM airband tuner (N = 2e7) with fixed squelch thresholds -- the path without a floor --
against set_floor + set_squelch(OverFloor(10)).  Median and IQR.  Prints one JSON line and writes it to `--out` (default
profiles/floor_band.json).

    python tools/floor_band.py [--steps 50] [--rounds 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402

# name -> (M, half, buffer length whose spectrum is binned, calls per step)
SHAPES = {"airband_6250Hz": (3200, 64, 20_000_000, 20), "fine_833Hz": (24_000, 128, 20_000_000, 20), "large_2^20": (1 << 20, 512, 1 << 22, 1)}
GUARD, Q = 4, 250


def spread(v, unit="us", digits=2):
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return {"median_" + unit: round(float(q[2]), digits), "iqr_" + unit: [round(float(q[1]), digits), round(float(q[3]), digits)],
            "min_" + unit: round(float(q[0]), digits), "max_" + unit: round(float(q[4]), digits)}


def timed(fn, steps, reps=1):
    """Device time per call of each of `steps` steps of `reps` calls back to back, microseconds."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        for _ in range(reps):
            fn()
        b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) / reps for a, b in ev]


def rounds(fns, a, reps):
    """{name: times} of the callables, alternating block by block."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    out = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            out[k] += timed(fn, a.steps, reps)
    return out


def airband(N=20_000_000, C=760, B=25_000, A=8000):
    tuner = rc.Tuner(cuda=True)
    for f in workloads.channel_grid(C, B):
        tuner.add_channel(f, B, rc.AM(B, A, cuda=True))
    tuner.request_bandwidth(float(N))
    return tuner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floor_band.json"))
    a = ap.parse_args()
    lib = hip.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    result = {"guard": GUARD, "q": Q, "steps": a.steps, "rounds": a.rounds, "floor_run": {}}
    tuner = airband()
    x = torch.view_as_complex(torch.randn(20_000_000, 2, generator=g, device="cuda") * 0.25)
    tuner.load(x)
    wide = rc.Tuner(cuda=True)
    wide.add_channel(100.0e6, 200_000, None)
    wide.request_bandwidth(float(1 << 22))
    wide.load(torch.view_as_complex(torch.randn(1 << 22, 2, generator=g, device="cuda") * 0.25))

    for name, (M, half, N, reps) in SHAPES.items():
        t = tuner if N == 20_000_000 else wide
        h = t._ready()
        power = t.power_spectrum(M, numpy_output=False)
        copy, floor = torch.empty_like(power), torch.empty_like(power)
        over = torch.empty((M,), dtype=torch.uint8, device="cuda")
        nf = rc.NoiseFloor(N / M, half=half, guard=GUARD, quantile=Q / 1000.0)
        handle = nf._create(M)
        cell = torch.randint(0, M, (760,), generator=g, device="cuda", dtype=torch.int32)
        gain = torch.rand(760, generator=g, device="cuda")
        thr = torch.empty(760, dtype=torch.float32, device="cuda")
        fns = {
            "floor_run": lambda: hip.check(lib.rcfm_floor_run(handle.value, hip.ptr(power), 10.0, hip.ptr(floor), hip.ptr(over), hip.stream())),
            "memcpy_d2d": lambda: hip.check(lib.rcfm_memcpy_d2d(hip.ptr(copy), hip.ptr(power), 4 * M, hip.stream())),
            "power_spectrum": lambda: hip.check(lib.rcfm_tuner_power_spectrum(h, -(N // 2), N, M, hip.ptr(copy), None, hip.stream())),
            "thresholds": lambda: hip.check(lib.rcfm_floor_thresholds(hip.ptr(floor), M, hip.ptr(cell), hip.ptr(gain), 760, hip.ptr(thr), hip.stream())),
        }
        tm = rounds(fns, a, reps)
        med = {k: float(np.median(v)) for k, v in tm.items()}
        result["floor_run"][name] = {
            "cells": M, "half": half, "bins": N, "calls_per_step": reps, **{k: spread(v) for k, v in tm.items()},
            "lds_reads": 32 * 2 * (half - GUARD) * M,
            "lds_reads_per_ns": round(32 * 2 * (half - GUARD) * M / med["floor_run"] * 1e-3, 1),
            "floor_run_over_memcpy": round(med["floor_run"] / med["memcpy_d2d"], 2),
            "floor_run_over_power_spectrum": round(med["floor_run"] / med["power_spectrum"], 3)}

    # the step the floor joins: load + run_all with fixed thresholds against the floor's
    fixed = rc.tools.squelch.threshold_over_floor(tuner.levels(), 25_000, 10.0)
    nf = rc.NoiseFloor(6250.0, half=64, guard=GUARD, quantile=0.25)

    def step():
        tuner.load(x)
        tuner.run_all(numpy_output=False)

    t_fixed, t_floor = [], []
    for _ in range(a.rounds):
        tuner.set_squelch(fixed)
        tuner.set_floor(None)
        step()
        t_fixed += timed(step, max(a.steps // 5, 4))
        tuner.set_floor(nf)
        tuner.set_squelch(rc.OverFloor(10.0))
        step()
        t_floor += timed(step, max(a.steps // 5, 4))
    off, on = float(np.median(t_fixed)), float(np.median(t_floor))
    result["airband_step"] = {"fixed_thresholds": spread(t_fixed), "over_floor": spread(t_floor), "added_us": round(on - off, 1),
                              "added_share": round((on - off) / off, 4)}
    line = json.dumps(result)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
