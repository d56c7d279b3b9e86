#!/usr/bin/env python3
"""What a buffer costs on its way out: float32 audio of every channel copied after the step (run_all) against int16 PCM of the
open channels, packed on the device and drained under the next buffer's kernels (run_all_packed + Drain).  GPU box.

Two geometries: the airband one (N = 2e7, 760 AM channels of 25 kHz -> 8 kHz) and cfg4 (N = 2.4e8, 1024 WBFM channels of
240 kHz -> 48 kHz), the input device-resident.  Wall time per buffer of the loop load -> run -> audio on the host, blocks of
`--fed` buffers, the forms alternating:
    compute        load + run_all(numpy_output=False), nothing brought back: the floor
    a_run_all      load + run_all() returning numpy: every row as float32, synchronously behind the step (the path before
                   run_all_packed existed, unchanged)
    b_s16_all      load + run_all_packed(int16, drain): every channel open
    c_s16_tenth    the same with one channel in ten open (thresholds of 0 and inf)
    d_f32_tenth    float32 compaction, one channel in ten open
With device events, alternating: rcfm_audio_pack (scan + pack) for int16 and float32, all open and a tenth open, next to
rcfm_memcpy_d2d of the same number of bytes read plus written; and the device-to-host copy of the int16 block into
page-locked memory.  Median and IQR.  Prints one JSON line and writes it to `--out` (default profiles/egress_band.json).

    python tools/egress_band.py [--steps 20] [--rounds 3] [--fed 8] [--sizes 20000000,240000000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import radiocore as rc  # noqa: E402
import workloads  # noqa: E402
from radiocore._internal import hip  # noqa: E402
from radiocore.tools import Drain  # noqa: E402

GEOMETRY = {20_000_000: (760, 25_000, 8_000, 25_000, "AM"), 240_000_000: (1024, 240_000, 48_000, 200_000, "WBFM")}


def spread(v, unit="ms", digits=4):
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return {"median_" + unit: round(float(q[2]), digits), "iqr_" + unit: [round(float(q[1]), digits), round(float(q[3]), digits)],
            "min_" + unit: round(float(q[0]), digits), "max_" + unit: round(float(q[4]), digits)}


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def measure(n, a):
    lib = hip.lib()
    C, B, A, raster, kind = GEOMETRY[n]
    ch = 2 if kind == "WBFM" else 1
    tuner = rc.Tuner(cuda=True)
    for f in workloads.channel_grid(C, raster):
        tuner.add_channel(f, B, getattr(rc, kind)(B, A, cuda=True))
    tuner.request_bandwidth(float(n))
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    x = torch.view_as_complex(torch.randn(n, 2, generator=g, device="cuda") * 0.25)
    tenth = np.where(np.arange(C) % 10 == 3, 0.0, np.inf).astype(np.float32)       # open iff level >= 0: one in ten
    n_tenth = int(np.sum(tenth == 0.0))
    s16, f32 = rc.PCM("int16"), rc.PCM("float32")
    drains = {"int16": Drain(C, (A, ch), "int16", depth=2), "float32": Drain(C, (A, ch), "float32", depth=2)}
    seen = {}

    def compute(k):
        for _ in range(k):
            tuner.load(x)
            tuner.run_all(numpy_output=False)

    def run_all(k):
        for _ in range(k):
            tuner.load(x)
            seen["a"] = tuner.run_all().shape[0]

    def drained(pcm, name):
        def loop(k):
            drain = drains[pcm.dtype.name]
            for i in range(k):
                tuner.load(x)
                tuner.run_all_packed(pcm, drain=drain)
                if i > 0:
                    with drain.next() as (index, audio):
                        seen[name] = audio.shape[0]
            with drain.next() as (index, audio):
                seen[name] = audio.shape[0]
        return loop

    forms = [("compute", None, compute), ("a_run_all", None, run_all), ("b_s16_all", None, drained(s16, "b")),
             ("c_s16_tenth", tenth, drained(s16, "c")), ("d_f32_tenth", tenth, drained(f32, "d"))]

    def wall(threshold, loop, k):
        tuner.set_squelch(threshold)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop(k)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    for _, thr, loop in forms:
        wall(thr, loop, 3)
    ms = {name: [] for name, _, _ in forms}
    for _ in range(a.rounds):
        for name, thr, loop in forms:              # alternating: every form sees the same machine state
            ms[name].append(wall(thr, loop, a.fed))
    out = {"N": n, "channels": C, "B": B, "A": A, "audio_channels": ch, "demodulator": kind, "open_tenth": n_tenth,
           "rows_seen": dict(seen), "wall_ms_per_buffer": {k: {"blocks": [round(v, 3) for v in vs], "median_ms": round(float(np.median(vs)), 3)}
                                                           for k, vs in ms.items()}}
    note("N = %d: wall loops done" % n)

    # ---- the pack alone against a device copy of the same bytes, and the copy to the host ----
    tuner.set_squelch(None)
    tuner.load(x)
    audio = tuner.run_all(numpy_output=False)
    row = A * ch
    s = hip.stream()
    mask = torch.from_numpy((tenth == 0.0).astype(np.uint8)).cuda()
    packed = hip.empty((C, A, ch), torch.float32)
    scratch = hip.empty((C, A, ch), torch.float32)
    index, n_open = hip.empty((C,), torch.int32), hip.empty((1,), torch.int32)
    pinned = torch.empty(C * row, dtype=torch.int16).pin_memory()

    def pack(fmt, m):
        return lambda: hip.check(lib.rcfm_audio_pack(hip.ptr(audio), None if m is None else hip.ptr(m), C, row, fmt, 32767.0,
                                                     hip.ptr(packed), hip.ptr(index), hip.ptr(n_open), s))

    def d2d(nbytes):
        return lambda: hip.check(lib.rcfm_memcpy_d2d(hip.ptr(scratch), hip.ptr(audio), ctypes.c_size_t(nbytes // 2), s))

    moved = {"pack_s16_all": 6 * C * row, "pack_f32_all": 8 * C * row, "pack_s16_tenth": 6 * n_tenth * row,
             "pack_f32_tenth": 8 * n_tenth * row}
    steps = {"pack_s16_all": pack(hip.RCFM_PCM_S16, None), "d2d_s16_all": d2d(moved["pack_s16_all"]),
             "pack_f32_all": pack(hip.RCFM_PCM_F32, None), "d2d_f32_all": d2d(moved["pack_f32_all"]),
             "pack_s16_tenth": pack(hip.RCFM_PCM_S16, mask), "d2d_s16_tenth": d2d(moved["pack_s16_tenth"]),
             "pack_f32_tenth": pack(hip.RCFM_PCM_F32, mask), "d2d_f32_tenth": d2d(moved["pack_f32_tenth"]),
             "d2h_s16_all": lambda: hip.check(lib.rcfm_memcpy_d2h(ctypes.c_void_p(pinned.data_ptr()), hip.ptr(packed),
                                                                  ctypes.c_size_t(2 * C * row), s))}
    for k in ("d2d_s16_all", "d2d_f32_all", "d2d_s16_tenth", "d2d_f32_tenth"):
        moved[k] = moved["pack" + k[3:]]
    moved["d2h_s16_all"] = 2 * C * row
    for _ in range(3):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in steps}
    for _ in range(a.steps):
        for k, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ev[k].append(e0.elapsed_time(e1))
    out["device_events"] = {}
    for k, v in ev.items():
        block = spread(v)
        block["bytes_moved"] = int(moved[k])
        block["GBps"] = round(moved[k] / (float(np.median(v)) * 1e-3) / 1e9, 1)
        out["device_events"][k] = block
    for d in drains.values():
        d.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fed", type=int, default=8)
    ap.add_argument("--sizes", default="20000000,240000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "egress_band.json"))
    a = ap.parse_args()
    result = {"config": {"steps": a.steps, "rounds": a.rounds, "buffers_per_block": a.fed, "device": torch.cuda.get_device_name(0)},
              "sizes": []}
    for n in [int(v) for v in a.sizes.split(",")]:
        result["sizes"].append(measure(n, a))
        torch.cuda.empty_cache()
    text = json.dumps(result)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
