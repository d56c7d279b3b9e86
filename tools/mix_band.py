#!/usr/bin/env python3
"""What the audio buses cost: rcfm_mix_run on the airband's audio against a pack and a device copy of the same rows, and the
airband step with and without a mixer.  GPU box.

Audio [760][8000][1] float32 (the AM airband), one and four stereo buses over all 760 channels (a quarter of the channels
each, in channel order, for four), with 12 of the 760 channels open -- the monitor's steady state -- and with all of them
open.  Alternating, `--rounds` blocks of `--steps` timed steps each, a step being `--calls` calls back to back between two
device events:
    mix_run      rcfm_mix_run: reads the open rows once, writes M rows of [8000][2]
    audio_pack   rcfm_audio_pack (float32) of the same open rows: reads and writes each once
    memcpy_d2d   rcfm_memcpy_d2d of as many bytes as the open rows hold
and load + run_all of the 760-channel AM airband tuner (N = 2e7) behind a level squelch that leaves the same 12 channels
open, without a mixer against set_mix of the four buses.  Median and IQR.  Prints one JSON line and writes it to `--out` (default profiles/mix_band.json).

    python tools/mix_band.py [--steps 50] [--rounds 5] [--calls 20]
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

C, A = 760, 8000


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


def buses(M, rng):
    """M buses over all C channels, a run of consecutive channels each, gains over -12 .. +6 dB, panned at random."""
    edges = np.linspace(0, C, M + 1).astype(int)
    return [rc.Bus.of(np.arange(edges[m], edges[m + 1]), gain_db=rng.uniform(-12.0, 6.0, edges[m + 1] - edges[m]),
                      pan=rng.uniform(-1.0, 1.0, edges[m + 1] - edges[m])) for m in range(M)]


def airband(N=20_000_000, B=25_000):
    tuner = rc.Tuner(cuda=True)
    for f in workloads.channel_grid(C, B):
        tuner.add_channel(f, B, rc.AM(B, A, cuda=True))
    tuner.request_bandwidth(float(N))
    return tuner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_band.json"))
    a = ap.parse_args()
    lib = hip.lib()
    rng = np.random.default_rng(11)
    g = torch.Generator(device="cuda").manual_seed(7)
    audio = torch.randn(C, A, 1, generator=g, device="cuda") * 0.1
    packed, copy = torch.empty_like(audio), torch.empty_like(audio)
    index = torch.empty((C,), dtype=torch.int32, device="cuda")
    n_open = torch.empty((1,), dtype=torch.int32, device="cuda")
    masks = {"12_open": np.zeros(C, np.uint8), "all_open": np.ones(C, np.uint8)}
    masks["12_open"][rng.choice(C, 12, replace=False)] = 1
    result = {"channels": C, "audio": A, "steps": a.steps, "rounds": a.rounds, "calls_per_step": a.calls, "mix_run": {}}
    for M in (1, 4):
        mixer = rc.Mixer(buses(M, rng), stereo=True)
        handle = mixer._create(*mixer._split(((0, C),), C)[1][0])
        out = torch.empty((M, A, 2), dtype=torch.float32, device="cuda")
        active = torch.empty((M,), dtype=torch.int32, device="cuda")
        bus_open = torch.empty((M,), dtype=torch.uint8, device="cuda")
        for name, mask in masks.items():
            opened = hip.to_device(mask, torch.uint8)
            rows = int(mask.sum())
            nbytes = 4 * A * rows
            fns = {
                "mix_run": lambda: hip.check(lib.rcfm_mix_run(handle.value, 0, C, A, 1, hip.ptr(audio), hip.ptr(opened), hip.ptr(out),
                                                              hip.ptr(active), hip.ptr(bus_open), hip.stream())),
                "audio_pack": lambda: hip.check(lib.rcfm_audio_pack(hip.ptr(audio), hip.ptr(opened), C, A, hip.RCFM_PCM_F32, 1.0,
                                                                    hip.ptr(packed), hip.ptr(index), hip.ptr(n_open), hip.stream())),
                "memcpy_d2d": lambda: hip.check(lib.rcfm_memcpy_d2d(hip.ptr(copy), hip.ptr(audio), nbytes, hip.stream())),
            }
            tm = rounds(fns, a, a.calls)
            med = {k: float(np.median(v)) for k, v in tm.items()}
            result["mix_run"]["%d_bus%s_%s" % (M, "es" if M > 1 else "", name)] = {
                "buses": M, "open_rows": rows, "bytes_read": nbytes, "bytes_written": 4 * A * 2 * M,
                **{k: spread(v) for k, v in tm.items()},
                "mix_read_GB_per_s": round(nbytes / med["mix_run"] * 1e-3, 1),
                "mix_run_over_audio_pack": round(med["mix_run"] / med["audio_pack"], 2),
                "mix_run_over_memcpy": round(med["mix_run"] / med["memcpy_d2d"], 2)}

    # the step the mixer joins: load + run_all behind a level squelch, without and with the four buses
    tuner = airband()
    x = torch.view_as_complex(torch.randn(20_000_000, 2, generator=g, device="cuda") * 0.25)
    tuner.load(x)
    thresholds = np.full(C, np.inf, np.float32)                # the band is noise: 12 channels open at any level, the rest never
    thresholds[masks["12_open"] != 0] = 0.0
    tuner.set_squelch(thresholds)
    mixer = rc.Mixer(buses(4, rng), stereo=True)

    def step():
        tuner.load(x)
        tuner.run_all(numpy_output=False)

    t_off, t_on = [], []
    for _ in range(a.rounds):
        tuner.set_mix(None)
        step()
        t_off += timed(step, max(a.steps // 5, 4))
        tuner.set_mix(mixer)
        step()
        t_on += timed(step, max(a.steps // 5, 4))
    off, on = float(np.median(t_off)), float(np.median(t_on))
    result["airband_step"] = {"without_mixer": spread(t_off), "with_4_buses": spread(t_on), "added_us": round(on - off, 1),
                              "added_share": round((on - off) / off, 4), "open_channels": int(tuner.open_mask().sum())}
    line = json.dumps(result)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
