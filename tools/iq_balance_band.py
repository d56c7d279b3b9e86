#!/usr/bin/env python3
"""What the IQ balance costs per load (rcfm_tuner_iq_estimate, rcfm_tuner_iq_correct, rcfm_tuner_set_iq_balance).  GPU box.

Two geometries: the airband one (N = 2e7, 760 channels of 25 kHz) and cfg4 (N = 2.4e8, 1024 channels of 240 kHz).  For each,
in one process, on device-resident buffers (noise at a quarter of full scale, complex64 and cu8):
    load, load_cu8              rcfm_tuner_load / rcfm_tuner_load_raw with the balance off: what a load costs without it
    estimate                    rcfm_tuner_iq_estimate over all pairs of the loaded spectrum (reads 8 n bytes)
    correct                     rcfm_tuner_iq_correct of the loaded spectrum (reads and writes 16 n bytes, plus the halos)
    both                        the two queued back to back, as the auto mode queues them
    load_fixed, load_auto       rcfm_tuner_load of a handle set to fixed / auto mode: the FFT with the work queued behind it
    load_cu8_auto               rcfm_tuner_load_raw (cu8) of the auto handle
Each step is timed with device events, `--steps` alternating rounds, the whole series `--series` times: median and IQR per
step and series.  `--lib PATH` runs what an older build of the library exports (the parent commit's: load and load_cu8 only)
so that its load can stand next to this build's in one file (`--merge FILE` stores it under "parent"; several files: under
"parent", "loads_only", ... in the order given as NAME=FILE); `--loads-only` runs that same two-step sequence on this build:
with the other steps in the rotation a load finds another cache state and its time is not the parent's to compare with.  Prints one JSON line and writes it to `--out`.

    python tools/iq_balance_band.py [--steps 30] [--warmup 5] [--series 2] [--sizes 20000000,240000000] [--lib PATH]
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

import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402

GEOMETRY = {20_000_000: (760, 25_000, 25_000), 240_000_000: (1024, 240_000, 200_000)}     # channels, bandwidth, raster
BETA = (-0.0244, -0.0262)


def spread(v):
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return {"median_ms": round(float(q[2]), 4), "iqr_ms": [round(float(q[1]), 4), round(float(q[3]), 4)],
            "min_ms": round(float(q[0]), 4), "max_ms": round(float(q[4]), 4)}


def measure(n, a, lib, have_balance):
    C, B, raster = GEOMETRY[n]

    def handle(mode):
        t = rc.Tuner(cuda=True)
        for f in workloads.channel_grid(C, raster):
            t.add_channel(f, B, None)
        t.request_bandwidth(float(n))
        h = t._device_tuner(n)
        if mode is not None:
            hip.check(lib.rcfm_tuner_set_iq_balance(h, mode, BETA[0], BETA[1], 1))
        return t, h
    s = hip.stream()
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    cu8 = (torch.randn(n, 2, generator=g, device="cuda") * 32 + 128).round_().clamp_(0, 255).to(torch.uint8)
    wide = hip.empty((n,), torch.complex64)
    hip.check(lib.rcfm_iq_convert(hip.RCFM_IQ_CU8, ctypes.c_size_t(n), hip.ptr(cu8), hip.ptr(wide), s))
    keep = [handle(None)]
    plain = keep[0][1]
    halo, nn = ctypes.c_int64(), ctypes.c_int64()
    hip.check(lib.rcfm_tuner_spectrum_layout(plain, ctypes.byref(halo), ctypes.byref(nn)))
    steps = {"load": lambda: hip.check(lib.rcfm_tuner_load(plain, hip.ptr(wide), s)),
             "load_cu8": lambda: hip.check(lib.rcfm_tuner_load_raw(plain, hip.RCFM_IQ_CU8, hip.ptr(cu8), s))}
    if have_balance and not a.loads_only:
        keep += [handle(hip.RCFM_IQ_BALANCE_FIXED), handle(hip.RCFM_IQ_BALANCE_AUTO)]
        fixed, auto = keep[1][1], keep[2][1]
        beta = torch.tensor(BETA, dtype=torch.float32, device="cuda")
        est = torch.empty(2, dtype=torch.float32, device="cuda")
        last = (n - 1) // 2

        def estimate():
            hip.check(lib.rcfm_tuner_iq_estimate(plain, 1, last, None, hip.ptr(est), s))

        def correct(b=beta):
            hip.check(lib.rcfm_tuner_iq_correct(plain, hip.ptr(b), 1, s))

        def both():
            estimate()
            correct(est)
        steps.update({"estimate": estimate, "correct": correct, "both": both,
                      "load_fixed": lambda: hip.check(lib.rcfm_tuner_load(fixed, hip.ptr(wide), s)),
                      "load_auto": lambda: hip.check(lib.rcfm_tuner_load(auto, hip.ptr(wide), s)),
                      "load_cu8_auto": lambda: hip.check(lib.rcfm_tuner_load_raw(auto, hip.RCFM_IQ_CU8, hip.ptr(cu8), s))})
    for _ in range(a.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    out = {"N": n, "channels": C, "B": B, "halo": int(halo.value),
           "algorithmic_bytes": {"estimate": 8 * n, "correct": 16 * n + 16 * int(halo.value)}, "series": []}
    for _ in range(a.series):
        ms = {k: [] for k in steps}
        for _ in range(a.steps):
            for k, fn in steps.items():              # alternating: every step sees the same machine state
                if k in ("estimate", "correct", "both"):
                    steps["load"]()                  # a fresh spectrum under every pass (repeated corrections would compound)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        block = {k: spread(v) for k, v in ms.items()}
        for k in ("estimate", "correct"):
            if k in block:
                block[k]["TBps"] = round(out["algorithmic_bytes"][k] / (block[k]["median_ms"] * 1e-3) / 1e12, 3)
        if "load_auto" in block:
            block["auto_cost_ms"] = round(block["load_auto"]["median_ms"] - block["load"]["median_ms"], 4)
            block["fixed_cost_ms"] = round(block["load_fixed"]["median_ms"] - block["load"]["median_ms"], 4)
        out["series"].append(block)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--series", type=int, default=2)
    ap.add_argument("--sizes", default="20000000,240000000")
    ap.add_argument("--lib", default=None, help="an older build of librcfm.so: only the steps it exports are run")
    ap.add_argument("--loads-only", action="store_true", help="load and load_cu8 alone: the sequence an older build runs")
    ap.add_argument("--merge", default=None, help="a result of --lib to store under 'parent' in this run's output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_balance_band.json"))
    a = ap.parse_args()
    if a.lib:
        hip._lib = hip.load_library(a.lib, strict=False)
    lib = hip.lib()
    have_balance = hasattr(lib, "rcfm_tuner_set_iq_balance")
    result = {"config": {"steps": a.steps, "warmup": a.warmup, "series": a.series, "device": torch.cuda.get_device_name(0),
                         "library": "this build" if not a.lib else "an older build (--lib)"}, "sizes": []}
    for n in [int(v) for v in a.sizes.split(",")]:
        result["sizes"].append(measure(n, a, lib, have_balance))
        torch.cuda.empty_cache()
    for item in (a.merge.split(",") if a.merge else []):
        name, _, path = item.rpartition("=")
        with open(path) as f:
            result[name or "parent"] = json.load(f)
    text = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
