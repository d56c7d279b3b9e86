#!/usr/bin/env python3
"""The subcarrier tap on the headline geometry: 1024 WBFM channels of 240 kHz in a 240 MSPS buffer (bench.py's cfg4), the
57 kHz tap with 241 taps down to 9 600 samples per channel.  GPU box.

One Tuner, one loaded spectrum; two steps alternate in one process:
    subcarrier   rcfm_pipeline_subcarrier over all channels: the Tuner's inverse FFT to phases, then the tap kernel
    wbfm         rcfm_pipeline_run with the WBFM demodulator over all channels -- the yardstick
Each step is timed with device events (profiler off), `--steps` alternating rounds, the whole series `--series` times:
median and IQR per step and series.  A further series with the library's stage profiler on for the Tuner's inverse FFT alone
(its own event pair around those launches) splits the tap step into "inverse FFT to phases" and the RESIDUAL, step minus
inverse FFT: the tap kernel plus the launch gap and the profiler's events, an upper bound of the kernel's time.  The kernel
itself is event-bracketed in its from-samples form: `rcfm_subcarrier_run` on the samples `rcfm_tuner_run` left, one launch,
8B + 8R bytes per channel instead of 4B + 8R.  Prints one JSON line.

    python tools/subcarrier_band.py [--steps 50] [--warmup 5] [--series 2] [--channels 1024]
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
from radiocore._internal import hip  # noqa: E402
from radiocore.tools import rds  # noqa: E402
from workloads_device import synth_wideband_on_device  # noqa: E402

B, A, RASTER = 240_000, 48_000, 200_000
R, F, T = 9_600, 57_000, 241


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--series", type=int, default=2)
    ap.add_argument("--channels", type=int, default=1024)
    a = ap.parse_args()
    C = a.channels
    N = 240_000_000 if C > 100 else 2_400_000 * max(1, C // 8)
    lib = hip.lib()
    x, centres, f_in = synth_wideband_on_device(N, C, B, RASTER, "WBFM")
    tuner = rc.Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, B, rc.WBFM(B, A, cuda=True))
    tuner.request_bandwidth(float(N))
    assert tuner.input_frequency == f_in
    tuner.load(x)
    handle = tuner._ready()
    kind, _, _, tau = tuner._plan_uniform()
    demod = tuner._batched_demod(kind, B, A, tau, 0)
    tap = rc.Subcarrier(B, R, F, rds.taps(B, R, T), cuda=True)._create(C, 0)
    audio = torch.empty((C, A, 2), dtype=torch.float32, device="cuda")
    y = torch.empty((C, R), dtype=torch.complex64, device="cuda")
    s = hip.stream()

    def subcarrier():
        hip.check(lib.rcfm_pipeline_subcarrier(handle, tap.value, 0, C, hip.ptr(y), s))

    def wbfm():
        hip.check(lib.rcfm_pipeline_run(handle, demod, 0, C, hip.ptr(audio), s))

    iq = torch.empty((C, B), dtype=torch.complex64, device="cuda")
    hip.check(lib.rcfm_tuner_run(handle, 0, C, hip.ptr(iq), s))

    def from_samples():
        hip.check(lib.rcfm_subcarrier_run(tap.value, C, hip.ptr(iq), hip.ptr(y), s))

    steps = {"subcarrier": subcarrier, "wbfm": wbfm}
    for _ in range(a.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.view_as_real(y)).all())

    def spread_of(v):
        q = np.percentile(v, [0, 25, 50, 75, 100])
        return {"median_ms": round(float(q[2]), 4), "iqr_ms": [round(float(q[1]), 4), round(float(q[3]), 4)],
                "min_ms": round(float(q[0]), 4), "max_ms": round(float(q[4]), 4)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"config": {"N": N, "B": B, "channels": C, "R": R, "f": F, "taps": T, "steps": a.steps, "warmup": a.warmup,
                      "series": a.series, "tap_bytes": (4.0 * B + 8.0 * R) * C, "tap_fma": 2.0 * T * R * C}, "series": []}
    for _ in range(a.series):
        ms = {k: [] for k in steps}
        for _ in range(a.steps):
            for k, fn in steps.items():              # alternating: every step sees the same machine state
                ms[k].append(timed(fn))
        block = {k: spread_of(v) for k, v in ms.items()}
        block["subcarrier_over_wbfm"] = round(block["subcarrier"]["median_ms"] / block["wbfm"]["median_ms"], 3)
        out["series"].append(block)
    # the split: the Tuner's inverse FFT reports to the stage profiler; what is left of the step is the tap kernel
    names = [lib.rcfm_profile_stage_name(i).decode() for i in range(lib.rcfm_profile_stage_count())]
    ifft = names.index("tuner_ifft_B") if "tuner_ifft_B" in names else None
    if ifft is not None:
        total, part = [], []
        lib.rcfm_profile_enable(ctypes.c_uint64(1 << ifft))
        for _ in range(a.steps):
            lib.rcfm_profile_reset()
            total.append(timed(subcarrier))
            msv, cnt = ctypes.c_double(), ctypes.c_int64()
            lib.rcfm_profile_read(ifft, ctypes.byref(msv), ctypes.byref(cnt))
            part.append(msv.value)
        lib.rcfm_profile_enable(ctypes.c_uint64(0))
        kernel = [t - p for t, p in zip(total, part)]
        out["split"] = {"step": spread_of(total), "ifft_to_phases": spread_of(part), "residual": spread_of(kernel)}
        k_ms = out["split"]["residual"]["median_ms"]
        out["split"]["residual_GBps"] = round(out["config"]["tap_bytes"] / (k_ms * 1e-3) / 1e9, 1)
        out["split"]["residual_GFMAps"] = round(out["config"]["tap_fma"] / (k_ms * 1e-3) / 1e9, 1)
    else:
        out["split"] = {"stages": names}
    # the kernel alone, from samples: one launch between two events
    for _ in range(a.warmup):
        from_samples()
    torch.cuda.synchronize()
    alone = spread_of([timed(from_samples) for _ in range(a.steps)])
    nbytes = (8.0 * B + 8.0 * R) * C
    out["kernel_from_samples"] = dict(alone, bytes=nbytes, GBps=round(nbytes / (alone["median_ms"] * 1e-3) / 1e9, 1),
                                      GFMAps=round(out["config"]["tap_fma"] / (alone["median_ms"] * 1e-3) / 1e9, 1))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
