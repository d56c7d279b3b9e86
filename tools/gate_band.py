#!/usr/bin/env python3
"""What the frame gate costs: rcfm_frame_power and rcfm_gate_apply on the airband shapes, with device events.  GPU box.

Alternating, `--rounds` blocks of `--steps` timed steps each, a step being 20 calls back to back between two device events:
    frame_power   760 x 25 000 complex64 in frames of 500 (F = 50), and 64 x 240 000 complex64 in frames of 4800
    gate_apply    760 x 8000 float32, F = 50, with every frame closed (all stores), every frame open (nothing to do) and a
                  random half of the frames open
    memcpy_d2d    rcfm_memcpy_d2d of the same bytes: the device-copy yardstick (it reads them and writes them back)
    levels        rcfm_tuner_levels of the same channels from the loaded spectrum: the per-buffer squelch's read
    frame_levels  rcfm_tuner_frame_levels: the inverse pass into the scratch plus frame_power
and load + run_all of the 760-channel AM airband tuner (N = 2e7) with the gate off and on.  Median and IQR.  Prints one JSON
line and writes it to `--out` (default profiles/gate_band.json).

    python tools/gate_band.py [--steps 50] [--rounds 5]
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

FRAMES = 50
REPS = 20            # launches back to back between two device events: a launch of 10 us is not timed alone
SHAPES = {"airband_760x25000": (760, 25_000, 8000, 20_000_000, "AM"), "wide_64x240000": (64, 240_000, 48_000, 15_360_000, "WBFM")}


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


def rounds(fns, a):
    """{name: times} of the callables, alternating block by block."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    out = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            out[k] += timed(fn, a.steps, REPS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_band.json"))
    a = ap.parse_args()
    lib = hip.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    result = {"frames": FRAMES, "calls_per_step": REPS, "steps": a.steps, "rounds": a.rounds, "frame_power": {}, "gate_apply": {}}
    tuners = {}

    for name, (C, B, A, N, kind) in SHAPES.items():
        tuner = rc.Tuner(cuda=True)
        for f in workloads.channel_grid(C, B):
            tuner.add_channel(f, B, getattr(rc, kind)(B, A, cuda=True))
        tuner.request_bandwidth(float(N))
        x = torch.view_as_complex(torch.randn(N, 2, generator=g, device="cuda") * 0.25)
        tuner.load(x)
        tuners[name] = (tuner, x)
        h = tuner._ready()
        iq = tuner.run_channels(0, C)
        copy = torch.empty_like(iq)
        power = torch.empty((C, FRAMES), dtype=torch.float32, device="cuda")
        level = torch.empty((C,), dtype=torch.float32, device="cuda")
        nbytes = 8 * C * B
        fns = {
            "frame_power": lambda: hip.check(lib.rcfm_frame_power(hip.ptr(iq), C, B, 1, B // FRAMES, hip.ptr(power), hip.stream())),
            "memcpy_d2d": lambda: hip.check(lib.rcfm_memcpy_d2d(hip.ptr(copy), hip.ptr(iq), nbytes, hip.stream())),
            "levels": lambda: hip.check(lib.rcfm_tuner_levels(h, 0, C, hip.ptr(level), hip.stream())),
            "frame_levels": lambda: tuner.frame_levels(FRAMES, numpy_output=False),
        }
        t = rounds(fns, a)
        med = {k: float(np.median(v)) for k, v in t.items()}
        result["frame_power"][name] = {
            "rows": C, "samples": B, "frame": B // FRAMES, "bytes_read": nbytes, **{k: spread(v) for k, v in t.items()},
            "read_GBps": round(nbytes / med["frame_power"] * 1e-3, 1),
            "frame_power_over_memcpy": round(med["frame_power"] / med["memcpy_d2d"], 3),
            "frame_power_over_levels": round(med["frame_power"] / med["levels"], 3),
            "frame_levels_over_levels": round(med["frame_levels"] / med["levels"], 3)}

    # gate apply on the airband audio
    C, _, A, _, _ = SHAPES["airband_760x25000"]
    gate = rc.FrameGate(frames=FRAMES)
    handle = gate._create(C, A)
    audio = torch.randn(C, A, generator=g, device="cuda") * 0.2
    copy = torch.empty_like(audio)
    rng = np.random.default_rng(7)
    masks = {"all_closed": np.zeros((C, FRAMES + 1), np.uint8), "all_open": np.ones((C, FRAMES + 1), np.uint8),
             "half_open": rng.integers(0, 2, (C, FRAMES + 1)).astype(np.uint8)}
    dev = {k: torch.from_numpy(m).cuda() for k, m in masks.items()}
    fns = {k: (lambda m=m: hip.check(lib.rcfm_gate_apply(handle.value, hip.ptr(m), C, FRAMES, A, 1, hip.ptr(audio), hip.stream())))
           for k, m in dev.items()}
    fns["memcpy_d2d"] = lambda: hip.check(lib.rcfm_memcpy_d2d(hip.ptr(copy), hip.ptr(audio), 4 * C * A, hip.stream()))
    t = rounds(fns, a)
    med = {k: float(np.median(v)) for k, v in t.items()}
    result["gate_apply"]["airband_760x8000"] = {
        "rows": C, "samples": A, "ramp": gate.ramp_samples(A), "bytes": 4 * C * A, **{k: spread(v) for k, v in t.items()},
        "all_closed_write_GBps": round(4 * C * A / med["all_closed"] * 1e-3, 1),
        "all_closed_over_memcpy": round(med["all_closed"] / med["memcpy_d2d"], 3),
        "half_open_over_memcpy": round(med["half_open"] / med["memcpy_d2d"], 3)}

    # the gate behind the run_all it follows
    tuner, x = tuners["airband_760x25000"]
    levels = tuner.levels()
    thr = rc.tools.squelch.threshold_over_floor(levels, 25_000, 6.0)

    def step():
        tuner.load(x)
        tuner.run_all(numpy_output=False)

    t_off, t_on = [], []
    for _ in range(a.rounds):
        tuner.set_gate(None)
        step()
        t_off += timed(step, max(a.steps // 5, 4))
        tuner.set_gate(gate, open=thr)
        step()
        t_on += timed(step, max(a.steps // 5, 4))
    off, on = float(np.median(t_off)), float(np.median(t_on))
    result["run_all_step"] = {"gate_off": spread(t_off), "gate_on": spread(t_on), "added_share": round((on - off) / off, 4)}
    line = json.dumps(result)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
