#!/usr/bin/env python3
"""SSB against AM and FM on the airband geometry: 760 channels of 25 kHz -> 8 kHz audio in a 20 MSPS buffer.  GPU box.

One Tuner, one loaded spectrum, one channel list; the step is what run_all launches after the load
(rcfm_pipeline_run over all channels) for four batched handles in alternation, in one process:
    USB         audio straight from the loaded spectrum (the spectrum-direct route)
    USB_general the same with RCFM_OPT_SSB_DIRECT off: tuner inverse FFT -> samples -> FFT_B -> IFFT_A
    AM, FM      the existing chains, as the yardstick
Pass 1 times the steps with device events (profiler off): median and IQR per handle.  Pass 2 reads the stage profile
of each handle and prices the SSB stages: the gather + IFFT_A reads 8 (A/2) and writes 4 A bytes per channel plus one
trip through the transform's scratch (16 A in all), ssb_tail reads and writes 4 A.  Prints one JSON line.

    python tools/ssb_band.py [--steps 50] [--warmup 10]
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
HBM_PEAK = 8e12


def stage_bytes(name, kind):
    """Algorithmic bytes of one channel's launch of stage `name`."""
    if name == "ssb_tail":
        return 8.0 * A                       # read and write the audio
    if kind.startswith("USB") and name == "ifft_A":
        # 8 (A/2) of spectrum bins in, the pair's packed scratch out and in (8 A per pair each way), 4 A of audio out
        return 4.0 * A + 8.0 * A + 4.0 * A
    if name == "envelope":
        return 12.0 * B
    if name == "am_tail":
        return 8.0 * A
    return bench.stage_bytes(name, N, B, A, "FM")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
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
    demods = {"USB": tuner._batched_demod(hip.RCFM_USB, B, A, 75e-6, 0)}
    tuner.set_kernel_options(ssb_direct=False)
    demods["USB_general"] = tuner._batched_demod(hip.RCFM_USB, B, A, 75e-6, 0)
    tuner.set_kernel_options()
    for k in ("AM", "FM"):
        demods[k] = tuner._batched_demod(getattr(hip, "RCFM_" + k), B, A, 75e-6, 0)
    audio = torch.empty((C, A, 1), dtype=torch.float32, device="cuda")
    s = hip.stream()

    def step(kind):
        hip.check(lib.rcfm_pipeline_run(handle, demods[kind], 0, C, hip.ptr(audio), s))

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

    def spread(v):
        q = np.percentile(v, [0, 25, 50, 75, 100])
        return {"median_ms": round(float(q[2]), 4), "iqr_ms": [round(float(q[1]), 4), round(float(q[3]), 4)],
                "min_ms": round(float(q[0]), 4), "max_ms": round(float(q[4]), 4)}

    out = {"config": {"N": N, "B": B, "A": A, "channels": C, "steps": a.steps, "warmup": a.warmup,
                      "step": "rcfm_pipeline_run over all channels after one tuner load"}}
    for k in demods:
        out[k] = spread(ms[k])
    med = {k: out[k]["median_ms"] for k in demods}
    out["direct_over_general"] = round(med["USB"] / med["USB_general"], 4)
    out["direct_over_am"] = round(med["USB"] / med["AM"], 4)
    out["direct_over_fm"] = round(med["USB"] / med["FM"], 4)

    # pass 2: the stage profile, each handle on its own (events on the stream slow the steps down)
    reps = 5
    out["stages"] = {}
    for k in demods:
        hip.check(lib.rcfm_profile_reset())
        hip.check(lib.rcfm_profile_enable(ctypes.c_uint64((1 << lib.rcfm_profile_stage_count()) - 1)))
        for _ in range(reps):
            step(k)
        torch.cuda.synchronize()
        prof = bench.read_profile(lib)
        hip.check(lib.rcfm_profile_enable(ctypes.c_uint64(0)))
        tab = {}
        for name, (_, t_ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
            if cnt == 0:
                continue
            by = stage_bytes(name, k) * C
            t = t_ms / reps
            tab[name] = {"ms": round(t, 4), "launches": cnt / reps, "algorithmic_bytes": by,
                         "TBps": round(by / (t * 1e-3) / 1e12, 3) if t else 0.0,
                         "frac_of_hbm_peak": round(by / (t * 1e-3) / HBM_PEAK, 3) if t else 0.0}
        out["stages"][k] = tab
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
