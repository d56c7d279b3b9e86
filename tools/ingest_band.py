#!/usr/bin/env python3
"""What a buffer costs on its way in, per sample format: complex64 against raw int16 / int8 / uint8 (rcfm_tuner_load_raw).
GPU box.

Two geometries: the airband one (N = 2e7, 760 AM channels of 25 kHz -> 8 kHz) and cfg4 (N = 2.4e8, 1024 WBFM channels of
240 kHz -> 48 kHz).  For each, in one process:
    load, load_cs16, load_cs8, load_cu8   the same handle's rcfm_tuner_load / rcfm_tuner_load_raw of device-resident
                                          buffers, alternating, timed with device events
    fed_c64, fed_cs16, fed_cs8            the host-fed step: Feeder (depth 2, page-locked sources) -> load / load_raw ->
                                          run_all, alternating blocks of `--fed` buffers, wall time per buffer
    host_convert                          numpy's int16 -> complex64 of one buffer on the host, the pass load_raw makes
                                          unnecessary (np.multiply into the output, and astype followed by a multiply)
`--steps` alternating rounds, the whole series `--series` times: median and IQR per step and series.  Prints one JSON line and
writes it to `--out` (default profiles/ingest_band.json).

    python tools/ingest_band.py [--steps 30] [--warmup 5] [--series 2] [--fed 12] [--sizes 20000000,240000000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402
from radiocore.tools import Buffer, Feeder  # noqa: E402

GEOMETRY = {20_000_000: (760, 25_000, 8_000, 25_000, "AM"), 240_000_000: (1024, 240_000, 48_000, 200_000, "WBFM")}
RAW = {"cs16": (hip.RCFM_IQ_CS16, torch.int16, "int16"), "cs8": (hip.RCFM_IQ_CS8, torch.int8, "int8"),
       "cu8": (hip.RCFM_IQ_CU8, torch.uint8, "uint8")}


def spread(v):
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return {"median_ms": round(float(q[2]), 4), "iqr_ms": [round(float(q[1]), 4), round(float(q[3]), 4)],
            "min_ms": round(float(q[0]), 4), "max_ms": round(float(q[4]), 4)}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def measure(n, a):
    lib = hip.lib()
    C, B, A, raster, kind = GEOMETRY[n]
    tuner = rc.Tuner(cuda=True)
    for f in workloads.channel_grid(C, raster):
        tuner.add_channel(f, B, getattr(rc, kind)(B, A, cuda=True))
    tuner.request_bandwidth(float(n))
    handle = tuner._device_tuner(n)
    s = hip.stream()
    # device-resident buffers: noise at a quarter of full scale
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    dev = {}
    for name, (fmt, tdt, _) in RAW.items():
        full = 32768 if name == "cs16" else 128
        v = (torch.randn(n, 2, generator=g, device="cuda") * (full / 4)).round_().clamp_(-full, full - 1)
        dev[name] = (v + 128 if name == "cu8" else v).to(tdt)
        del v
    wide = hip.empty((n,), torch.complex64)
    hip.check(lib.rcfm_iq_convert(hip.RCFM_IQ_CS16, ctypes.c_size_t(n), hip.ptr(dev["cs16"]), hip.ptr(wide), s))
    routes = {}
    for name, (fmt, _, _) in RAW.items():
        r = ctypes.c_int(-1)
        hip.check(lib.rcfm_tuner_load_route(handle, fmt, ctypes.byref(r)))
        routes[name] = r.value

    def loader(name):
        if name == "c64":
            return lambda x=wide: hip.check(lib.rcfm_tuner_load(handle, hip.ptr(x), s))
        fmt = RAW[name][0]
        return lambda x=dev[name]: hip.check(lib.rcfm_tuner_load_raw(handle, fmt, hip.ptr(x), s))

    steps = {"load": loader("c64"), "load_cs16": loader("cs16"), "load_cs8": loader("cs8"), "load_cu8": loader("cu8")}
    for _ in range(a.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()

    # page-locked sources, two per format (the feeder's copy of one runs under the kernels of the other)
    host = {}
    for name, src in (("c64", wide), ("cs16", dev["cs16"]), ("cs8", dev["cs8"])):
        dt, size = ("complex64", n) if name == "c64" else (RAW[name][2], 2 * n)
        host[name] = [Buffer(size, dt, cuda=True) for _ in range(2)]
        for b in host[name]:
            b.data[:] = src.reshape(-1).cpu().numpy()
        note("N = %d: %s sources pinned" % (n, name))
    feeders = {name: Feeder(host[name][0].size, host[name][0].dtype, depth=2) for name in host}

    def fed(name, k):
        """k buffers through the feeder -> load -> run_all; wall ms per buffer (the first copy is not hidden)."""
        f, src = feeders[name], host[name]
        load = tuner.load if name == "c64" else tuner.load_raw
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.submit(src[0].data)
        for i in range(k):
            if i + 1 < k:
                f.submit(src[(i + 1) % 2].data)
            with f.next() as x:
                load(x)
                tuner.run_all(numpy_output=False)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    for name in host:
        fed(name, 3)
    tuner.load(wide)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        tuner.run_all(numpy_output=False)
    e1.record()
    e1.synchronize()
    run_all_ms = e0.elapsed_time(e1) / 5

    out = {"N": n, "channels": C, "B": B, "A": A, "demodulator": kind, "route": routes,
           "h2d_bytes": {"c64": 8 * n, "cs16": 4 * n, "cs8": 2 * n}, "run_all_ms": round(run_all_ms, 4), "series": []}
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
        fed_ms = {name: [] for name in host}
        for _ in range(3):
            for name in host:
                fed_ms[name].append(fed(name, a.fed))
        for name, v in fed_ms.items():
            block["fed_" + name] = {"ms_per_buffer": [round(x, 3) for x in v], "median_ms": round(float(np.median(v)), 3),
                                    "GBps": round(out["h2d_bytes"][name] / (float(np.median(v)) * 1e-3) / 1e9, 2)}
        out["series"].append(block)
        note("N = %d: series done" % n)

    # the host's own conversion of one int16 buffer, pageable destination like any numpy result
    raw = host["cs16"][0].data
    dst = np.empty(n, np.complex64)
    one, two = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        np.multiply(raw, np.float32(2.0 ** -15), out=dst.view(np.float32), dtype=np.float32, casting="unsafe")
        one.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        dst.view(np.float32)[:] = raw.astype(np.float32) * np.float32(2.0 ** -15)
        two.append(1e3 * (time.perf_counter() - t0))
    out["host_convert"] = {"multiply_into_ms": round(float(np.median(one)), 1), "astype_then_multiply_ms": round(float(np.median(two)), 1)}
    for f in feeders.values():
        f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--series", type=int, default=2)
    ap.add_argument("--fed", type=int, default=12)
    ap.add_argument("--sizes", default="20000000,240000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_band.json"))
    a = ap.parse_args()
    result = {"config": {"steps": a.steps, "warmup": a.warmup, "series": a.series, "fed_buffers": a.fed,
                         "device": torch.cuda.get_device_name(0)}, "sizes": []}
    for n in [int(v) for v in a.sizes.split(",")]:
        result["sizes"].append(measure(n, a))
        torch.cuda.empty_cache()
    text = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
