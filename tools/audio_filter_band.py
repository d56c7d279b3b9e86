#!/usr/bin/env python3
"""The audio filter's kernel against a copy, the float32 pack and the AGC tail, on two geometries: the airband audio
(760 channels x 8000 samples) and 64 channels of 48 kHz stereo.  GPU box.

Per geometry six series alternate in one process: a device copy of the same bytes (the floor: one read and one write), a
float32 rcfm_audio_pack of the same rows, rcfm_agc in CARRIER mode (k_agc_tail: the same mapping with a scalar state and a
cheaper recurrence; stereo rows are taken as rows of 2 A samples), and rcfm_audio_filter_run with S = 1, 3 and 8 sections.
All run out of place from one source, so nothing decays towards zero over the repeats.  One timing is `reps` launches back
to back between two device events, divided by reps; 50 such steps per series, the whole round twice, median [IQR].
Then the step `load + run_all` of the airband Tuner (AM, 20 MSPS) with and without set_audio_filter(VOICE_AM),
alternating.  Writes profiles/audio_filter_band.json and prints it.

    python tools/audio_filter_band.py [--steps 50] [--warmup 10] [--reps 20] [--no-tuner] [--out profiles/audio_filter_band.json]
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

import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402
from radiocore.tools import audiofilter as af  # noqa: E402

GEOMETRIES = {"airband_760x8000": (760, 8000, 1), "stereo_64x48000x2": (64, 48000, 2)}
N, B, A, C = 20_000_000, 25000, 8000, 760
_dp = ctypes.POINTER(ctypes.c_double)


def spread(v):
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return {"median": round(float(q[2]), 3), "iqr": [round(float(q[1]), 3), round(float(q[3]), 3)],
            "min": round(float(q[0]), 3), "max": round(float(q[4]), 3)}


def filters(rate):
    """S -> sections: the de-emphasis; with the 300 Hz high-pass; eight sections (high-pass, low-pass of order 6, de-emphasis
    twice -- what matters here is their number)."""
    de, hp = af.AudioFilter.deemphasis(750e-6), af.AudioFilter.highpass(300.0)
    return {1: de.sections(rate), 3: (hp + de).sections(rate),
            8: (hp + af.AudioFilter.lowpass(3000.0, order=8) + de + de).sections(rate)}


def kernel_series(lib, count, n, ch, a):
    g = torch.Generator(device="cuda").manual_seed(1)
    x = 0.5 + 0.2 * torch.randn((count, n, ch), device="cuda", dtype=torch.float32, generator=g)
    y = torch.empty_like(x)
    s = hip.stream()
    nbytes = x.numel() * 4
    index = torch.empty((count,), dtype=torch.int32, device="cuda")
    n_open = torch.empty((1,), dtype=torch.int32, device="cuda")
    agc_state = torch.full((count,), -1.0, dtype=torch.float32, device="cuda")
    handles = {}
    for S, sos in filters(n).items():
        assert sos.shape[0] == S
        h = ctypes.c_void_p()
        hip.check(lib.rcfm_audio_filter_create(count, ch, S, np.ascontiguousarray(sos).ctypes.data_as(_dp), ctypes.byref(h)))
        handles[S] = hip.Handle(h, lib.rcfm_audio_filter_destroy)
    launch = {
        "copy": lambda: hip.check(lib.rcfm_memcpy_d2d(hip.ptr(y), hip.ptr(x), nbytes, s)),
        "pack_f32": lambda: hip.check(lib.rcfm_audio_pack(hip.ptr(x), None, count, n * ch, hip.RCFM_PCM_F32, 1.0, hip.ptr(y),
                                                          hip.ptr(index), hip.ptr(n_open), s)),
        "agc_carrier": lambda: hip.check(lib.rcfm_agc(count, n * ch, hip.RCFM_AGC_CARRIER, 2400.0, 1.0, 1e-3, hip.ptr(agc_state),
                                                      hip.ptr(x), hip.ptr(y), s)),
    }
    for S, h in handles.items():
        launch["filter_S%d" % S] = (lambda hv: lambda: hip.check(lib.rcfm_audio_filter_run(hv, 0, count, n, hip.ptr(x), hip.ptr(y),
                                                                                         None, s)))(h.value)
    out = []
    for series in range(2):
        for _ in range(a.warmup):
            for k in launch:
                launch[k]()
        torch.cuda.synchronize()
        us = {k: [] for k in launch}
        for _ in range(a.steps):
            for k in launch:                 # alternating: every series sees the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    launch[k]()
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        rec = {"us": {k: spread(v) for k, v in us.items()}}
        for S in handles:
            k = "filter_S%d" % S
            rec[k + "_over_copy"] = round(rec["us"][k]["median"] / rec["us"]["copy"]["median"], 3)
            rec[k + "_over_agc"] = round(rec["us"][k]["median"] / rec["us"]["agc_carrier"]["median"], 3)
            rec[k + "_GBps"] = round(2.0 * nbytes / rec["us"][k]["median"] * 1e-3, 1)
        rec["copy_GBps"] = round(2.0 * nbytes / rec["us"]["copy"]["median"] * 1e-3, 1)
        out.append(rec)
    return {"bytes_read_plus_written": 2 * nbytes, "series": out}


def tuner_step(a):
    centres = workloads.channel_grid(C, B)
    tuners = {}
    for name, voice in (("plain", None), ("voice_am", af.VOICE_AM)):
        t = rc.Tuner(cuda=True)
        for f in centres:
            t.add_channel(f, B, rc.AM(B, A, cuda=True))
        t.request_bandwidth(float(N))
        t.set_audio_filter(voice)
        tuners[name] = t
    x = hip.to_device(workloads.wideband(N, tuners["plain"].input_frequency, centres, B, gain=0.05, stereo=False, deviation=0.2 * B))
    out = []
    for series in range(2):
        for _ in range(a.warmup):
            for t in tuners.values():
                t.load(x)
                t.run_all(numpy_output=False)
        torch.cuda.synchronize()
        ms = {k: [] for k in tuners}
        for _ in range(a.steps):
            for k, t in tuners.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t.load(x)
                t.run_all(numpy_output=False)
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        rec = {"step_ms": {k: spread(v) for k, v in ms.items()}}
        rec["voice_am_over_plain"] = round(rec["step_ms"]["voice_am"]["median"] / rec["step_ms"]["plain"]["median"], 4)
        out.append(rec)
    return {"config": {"N": N, "B": B, "A": A, "channels": C, "demodulator": "AM", "filter": "VOICE_AM (4 sections)",
                       "step": "Tuner.load of a device buffer + run_all, device output"}, "series": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-tuner", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_filter_band.json"))
    a = ap.parse_args()
    lib = hip.lib()
    out = {"config": {"steps": a.steps, "warmup": a.warmup, "reps": a.reps,
                      "timing": "reps launches back to back between two device events, divided by reps; microseconds"},
           "kernels": {}}
    for name, (count, n, ch) in GEOMETRIES.items():
        out["kernels"][name] = kernel_series(lib, count, n, ch, a)
    if not a.no_tuner:
        out["tuner"] = tuner_step(a)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
