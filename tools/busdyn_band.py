#!/usr/bin/env python3
"""What the bus dynamics cost: rcfm_busdyn_run on the airband's buses against the mixer that feeds it and a device copy of
the same rows, and the airband step with and without the stage.  GPU box.

Two sizes of bus rows: 4 x 8000 x 2 (the airband monitor: four stereo buses over 760 AM channels, 12 of them open, blocks of
64 samples, 125 knots per bus) and 64 x 48 000 x 2 (64 stereo buses over 128 stereo channels of 48 000 samples, all open,
blocks of 384 samples).  The rows are noise with a burst over the ceiling in every bus, and the "everything else" buses are
ducked by the first one.  Alternating, `--rounds` blocks of `--steps` timed steps each, a step being `--calls` calls back to
back between two device events:
    busdyn_run   rcfm_busdyn_run: three launches; reads M rows and the tail, writes M rows and the tail
    mix_run      rcfm_mix_run, which wrote those rows
    memcpy_d2d   rcfm_memcpy_d2d of as many bytes as the M rows hold
and load + run_all of the 760-channel AM airband tuner (N = 2e7) behind a level squelch that leaves 12 channels open, with
four buses, without the stage against set_bus_dynamics(Limiter(), ducks).  Median and IQR.  Prints one JSON line and writes
it to `--out` (default profiles/busdyn_band.json).

    python tools/busdyn_band.py [--steps 50] [--rounds 5] [--calls 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import radiocore as rc  # noqa: E402
from mix_band import airband, rounds, spread, timed  # noqa: E402
from radiocore._internal import hip  # noqa: E402
from radiocore.tools import busdyn  # noqa: E402


def case(lib, rng, g, name, C, A, ch_in, M, n_open):
    """The three callables for M stereo buses over C channels of A samples, n_open of them open."""
    edges = np.linspace(0, C, M + 1).astype(int)
    law = dict(balance=0.0) if ch_in == 2 else dict(pan=0.0)
    mixer = rc.Mixer([rc.Bus.of(np.arange(edges[m], edges[m + 1]), gain_db=0.0, **law) for m in range(M)], stereo=True)
    mix = mixer._create(*mixer._split(((0, C),), C)[1][0])
    audio = torch.randn(C, A, ch_in, generator=g, device="cuda") * 0.1
    audio[:, A // 3:A // 3 + A // 8] *= 30.0                       # a burst over the ceiling in every channel
    mask = np.zeros(C, np.uint8)
    mask[rng.choice(C, n_open, replace=False)] = 1
    mask[edges[:-1]] = 1                                           # every bus has an open channel
    opened = hip.to_device(mask, torch.uint8)
    out = torch.empty((M, A, 2), dtype=torch.float32, device="cuda")
    wet, copy = torch.empty_like(out), torch.empty_like(out)
    active = torch.empty((M,), dtype=torch.int32, device="cuda")
    bus_open, open_out = torch.empty((M,), dtype=torch.uint8, device="cuda"), torch.empty((M,), dtype=torch.uint8, device="cuda")
    L, c, k = rc.Limiter().discretise(A)
    d, thr, hold = rc.Duck(0).discretise(A, L)
    key = np.array([-1] + [0] * (M - 1), np.int32)
    dyn = busdyn.create(M, 2, L, A, c, k, key, np.full(M, d, np.float32), np.full(M, thr, np.float32), np.full(M, hold, np.int32))
    nbytes = 4 * A * 2 * M
    fns = {
        "busdyn_run": lambda: hip.check(lib.rcfm_busdyn_run(dyn.value, A, hip.ptr(out), hip.ptr(bus_open), hip.ptr(wet),
                                                            hip.ptr(open_out), hip.stream())),
        "mix_run": lambda: hip.check(lib.rcfm_mix_run(mix.value, 0, C, A, ch_in, hip.ptr(audio), hip.ptr(opened), hip.ptr(out),
                                                      hip.ptr(active), hip.ptr(bus_open), hip.stream())),
        "memcpy_d2d": lambda: hip.check(lib.rcfm_memcpy_d2d(hip.ptr(copy), hip.ptr(out), nbytes, hip.stream())),
    }
    fns["mix_run"]()                                               # the rows the stage reads
    keep = (mixer, mix, dyn, audio, opened, out, wet, copy, active, bus_open, open_out)
    return fns, keep, {"name": name, "buses": M, "audio": A, "block": L, "knots_per_bus": -(-A // L), "open_channels": int(mask.sum()),
                       "row_bytes": nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "busdyn_band.json"))
    a = ap.parse_args()
    lib = hip.lib()
    rng = np.random.default_rng(12)
    g = torch.Generator(device="cuda").manual_seed(8)
    result = {"steps": a.steps, "rounds": a.rounds, "calls_per_step": a.calls, "busdyn_run": {}}
    for name, C, A, ch_in, M, n_open in (("4x8000x2", 760, 8000, 1, 4, 12), ("64x48000x2", 128, 48000, 2, 64, 128)):
        fns, keep, info = case(lib, rng, g, name, C, A, ch_in, M, n_open)
        tm = rounds(fns, a, a.calls)
        med = {k: float(np.median(v)) for k, v in tm.items()}
        result["busdyn_run"][name] = {**info, **{k: spread(v) for k, v in tm.items()},
                                      "busdyn_GB_per_s": round(2 * info["row_bytes"] / med["busdyn_run"] * 1e-3, 1),
                                      "busdyn_run_over_mix_run": round(med["busdyn_run"] / med["mix_run"], 2),
                                      "busdyn_run_over_memcpy": round(med["busdyn_run"] / med["memcpy_d2d"], 2)}
        del fns, keep
    # the step the stage joins: load + run_all behind a level squelch with four buses, without and with it
    C, A = 760, 8000
    tuner = airband()
    x = torch.view_as_complex(torch.randn(20_000_000, 2, generator=g, device="cuda") * 0.25)
    tuner.load(x)
    thresholds = np.full(C, np.inf, np.float32)                # the band is noise: 12 channels open at any level, the rest never
    thresholds[rng.choice(C, 12, replace=False)] = 0.0
    tuner.set_squelch(thresholds)
    edges = np.linspace(0, C, 5).astype(int)
    tuner.set_mix(rc.Mixer([rc.Bus.of(np.arange(edges[m], edges[m + 1]), name="bus %d" % m) for m in range(4)], stereo=True))
    ducks = {m: rc.Duck("bus 0") for m in (1, 2, 3)}

    def step():
        tuner.load(x)
        tuner.run_all(numpy_output=False)

    t_off, t_on = [], []
    for _ in range(a.rounds):
        tuner.set_bus_dynamics()
        step()
        t_off += timed(step, max(a.steps // 5, 4))
        tuner.set_bus_dynamics(rc.Limiter(), ducks)
        step()
        t_on += timed(step, max(a.steps // 5, 4))
    off, on = float(np.median(t_off)), float(np.median(t_on))
    result["airband_step"] = {"without_stage": spread(t_off), "with_limiter_and_ducks": spread(t_on), "added_us": round(on - off, 1),
                              "added_share": round((on - off) / off, 4), "open_channels": int(tuner.open_mask().sum())}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
