#!/usr/bin/env python3
"""What the noise blanker costs: rcfm_blanker_run over wideband buffers on the device, with device events.  GPU box.

Buffers: receiver noise with 200 three-sample pulses 35 dB over the RMS -- the airband buffer (n = 2e7) as complex64 and as
cs16, and n = 2.4e8 as complex64.  Per buffer, alternating, `--rounds` blocks of `--steps` timed calls each:
    median / absolute x in_place / out_of_place    rcfm_blanker_run (the default NoiseBlanker: L = 4096, W = 4, 12 dB)
    copy                                           rcfm_memcpy_d2d of the same buffer: the yardstick -- a read and a write,
                                                   the bytes an in-place median run moves as two reads
An in-place run blanks its buffer, so the buffer is restored from a pristine copy before every timed call, outside the
events.  Then load + run_all of the 760-channel AM airband tuner (N = 2e7, a device tensor: the blanker writes the tuner's
scratch) with the blanker off and on.  Median and IQR.  Prints one JSON line and writes it to `--out` (default
profiles/blanker_band.json).

    python tools/blanker_band.py [--steps 20] [--rounds 3]
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

C, A, B = 760, 8000, 25_000
PULSES, PULSE, OVER_DB = 200, 3, 35.0


def spread(v, unit="us", digits=1):
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return {"median_" + unit: round(float(q[2]), digits), "iqr_" + unit: [round(float(q[1]), digits), round(float(q[3]), digits)],
            "min_" + unit: round(float(q[0]), digits), "max_" + unit: round(float(q[4]), digits)}


def timed(fn, steps, prep=None):
    """Device time of each of `steps` calls, microseconds; `prep` runs before each, outside the events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        if prep is not None:
            prep()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def buffer(n, g, cs16=False):
    """Noise of RMS 0.05 with the pulses on it, complex64 [n] or int16 [n, 2], on the device."""
    x = torch.randn(n, 2, generator=g, device="cuda") * (0.05 / np.sqrt(2.0))
    at = torch.randint(0, n - PULSE, (PULSES,), generator=g, device="cuda")
    amp = 0.05 * 10.0 ** (OVER_DB / 20.0) / np.sqrt(2.0)
    for k in range(PULSE):
        x[at + k] = amp
    if cs16:
        return torch.clamp(torch.round(x * (32768.0 * 0.25)), -32768, 32767).to(torch.int16)
    return torch.view_as_complex(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blanker_band.json"))
    a = ap.parse_args()
    lib = hip.lib()
    g = torch.Generator(device="cuda").manual_seed(11)
    result = {"steps": a.steps, "rounds": a.rounds, "pulses": PULSES, "buffers": {}}
    for name, n, cs16 in (("airband_cf32", 20_000_000, False), ("airband_cs16", 20_000_000, True), ("n2.4e8_cf32", 240_000_000, False)):
        pristine = buffer(n, g, cs16)
        work, out = torch.empty_like(pristine), torch.empty_like(pristine)
        nbytes = pristine.numel() * pristine.element_size()
        fmt = hip.RCFM_IQ_CS16 if cs16 else hip.RCFM_IQ_CF32
        level = 0.05 ** 2 * (0.25 ** 2 if cs16 else 1.0)
        blankers = {"median": rc.NoiseBlanker(), "absolute": rc.NoiseBlanker(absolute=100.0 * level)}
        handles = {k: b._create(n) for k, b in blankers.items()}
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")

        def restore():
            hip.check(lib.rcfm_memcpy_d2d(hip.ptr(work), hip.ptr(pristine), ctypes.c_size_t(nbytes), hip.stream()))

        def copy():
            hip.check(lib.rcfm_memcpy_d2d(hip.ptr(out), hip.ptr(pristine), ctypes.c_size_t(nbytes), hip.stream()))

        def run(mode, in_place):
            dst = work if in_place else out
            return lambda: hip.check(lib.rcfm_blanker_run(handles[mode].value, fmt, n, hip.ptr(work), hip.ptr(dst), hip.ptr(stats),
                                                          hip.stream()))

        forms = {"%s_%s" % (m, "in_place" if ip else "out_of_place"): run(m, ip) for m in ("median", "absolute") for ip in (True, False)}
        times = {k: [] for k in list(forms) + ["copy"]}
        counts = {}
        for k, fn in forms.items():
            restore()
            fn()
            copy()
            counts[k] = [int(v) for v in stats.cpu()]
        for _ in range(a.rounds):
            for k, fn in forms.items():
                times[k] += timed(fn, a.steps, prep=restore)
                times["copy"] += timed(copy, a.steps, prep=restore)
        med_copy = float(np.median(times["copy"]))
        entry = {"n": n, "bytes": nbytes, "copy": spread(times["copy"]), "copy_GBps": round(2.0 * nbytes / med_copy * 1e-3, 1)}
        for k in forms:
            med = float(np.median(times[k]))
            entry[k] = dict(spread(times[k]), over_copy=round(med / med_copy, 3), hits=counts[k][0], blanked=counts[k][1])
        result["buffers"][name] = entry
        del pristine, work, out, handles
        torch.cuda.empty_cache()

    # the blanker ahead of the load it serves
    N = 20_000_000
    tuner = rc.Tuner(cuda=True)
    for f in workloads.channel_grid(C, B):
        tuner.add_channel(f, B, rc.AM(B, A, cuda=True))
    tuner.request_bandwidth(float(N))
    x = buffer(N, g)

    def step():
        tuner.load(x)
        tuner.run_all(numpy_output=False)

    t_off, t_on = [], []
    nb = rc.NoiseBlanker()
    for _ in range(a.rounds):
        tuner.set_blanker(None)
        step()
        t_off += timed(step, max(a.steps // 2, 4))
        tuner.set_blanker(nb)
        step()
        t_on += timed(step, max(a.steps // 2, 4))
    off, on = float(np.median(t_off)), float(np.median(t_on))
    result["load_run_all"] = {"blanker_off": spread(t_off), "blanker_on": spread(t_on), "added_share": round((on - off) / off, 4),
                              "stats": list(tuner.blanker_stats())}
    print(json.dumps(result))
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
