#!/usr/bin/env python3
"""The buses of examples/airband_mix.py with four stations keyed at once on one of them, without and with bus dynamics, no
SDR or sound card.

The mixer's sum has unit gain: four tower stations talking over each other leave full scale, and the int16 payload of
`run_all_packed(PCM("int16"), buses=True)` is clipped.  `Tuner.set_bus_dynamics(Limiter())` turns the bus down 8 ms before
the peak arrives (include/rcfm.h, "bus dynamics"): no sample of the payload reaches +-32767.  A `Duck` on the "everything
else" bus, keyed by the tower bus, lowers it by 12 dB while the tower talks and for half a second after.  The tower stations
key up together 1.2 s into the three seconds and stop at 2.0 s; the other stations talk throughout.

    python examples/airband_mix_limited.py [--channels 760] [--rate 20000000] [--stations 12] [--small]
"""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AM, PCM, Bus, Duck, FrameGate, Limiter, Mixer, Tuner  # noqa: E402
from radiocore.tools import squelch  # noqa: E402

_spec = importlib.util.spec_from_file_location("airband_gate", os.path.join(ROOT, "examples", "airband_gate.py"))
airband_gate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(airband_gate)

CHANNEL, AUDIO, SECONDS, FRAMES = airband_gate.CHANNEL, airband_gate.AUDIO, airband_gate.SECONDS, airband_gate.FRAMES
OVER_FLOOR_DB = airband_gate.OVER_FLOOR_DB
SMALL = dict(channels=40, rate=1_000_000, stations=6)
TOWER, STANDBY = 4, 3          # channels of the tower group (stations) and of the standby bus (no station)
TALK = (1.2, 2.0)              # the tower stations, all four at once
GAIN = 32767.0                 # int16 per unit of audio: full scale is full scale


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def run(channels=760, rate=20_000_000, stations=12):
    """Three buffers through a tuner that mixes and one that mixes and limits.  Returns, for each, the peak and the count
    of samples at +-32767 in the int16 payloads, and the level of the processed "everything else" bus while the tower
    is quiet and while it talks."""
    first = 118_012_500.0                          # the centre of the first 25 kHz airband channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuners = []
    for _ in range(2):
        tuner = Tuner(cuda=True)
        for f in centres:
            tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
        tuner.request_bandwidth(float(rate))
        tuners.append(tuner)
    plain, limited = tuners
    rng = np.random.default_rng(123)
    chosen = sorted(int(i) for i in rng.choice(channels, stations, replace=False))
    tower_channels = chosen[:TOWER]
    on_air = {c: [TALK] if c in tower_channels else [(0.1, SECONDS - 0.2)] for c in chosen}
    standby_channels = [c for c in range(channels) if c not in on_air][:STANDBY]
    others = [c for c in range(channels) if c not in tower_channels and c not in standby_channels]
    buses = [Bus.of(tower_channels, gain_db=0.0, pan=np.linspace(-0.7, 0.7, len(tower_channels)), name="tower"),
             Bus.of(others, gain_db=-6.0, pan=0.0, name="everything else"),
             Bus.of(standby_channels, gain_db=0.0, pan=0.0, name="standby")]
    mixer = Mixer(buses, stereo=True)
    for t in tuners:
        t.set_mix(mixer)
    limited.set_bus_dynamics(Limiter(), ducks={"everything else": Duck("tower", depth_db=-12.0, threshold_db=-40.0, hold=0.5)})
    gate = FrameGate(frames=FRAMES, hang=0.25, lead=1, ramp=0.005)
    pcm = PCM("int16", GAIN)
    report = {"plain": {"peak": 0, "at_full_scale": 0}, "limited": {"peak": 0, "at_full_scale": 0}}
    rest = []
    for second in range(SECONDS):
        x = airband_gate.band(rate, centres, plain.input_frequency, on_air, second, rng)
        for t in tuners:
            t.load(x)
        if second == 0:
            thresholds = squelch.threshold_over_floor(plain.levels(), CHANNEL, OVER_FLOOR_DB)
            for t in tuners:
                t.set_gate(gate, open=thresholds)
        for name, t in (("plain", plain), ("limited", limited)):
            index, rows = t.run_all_packed(pcm, buses=True)
            if len(index):
                mag = np.abs(np.asarray(rows, np.int32))
                report[name]["peak"] = max(report[name]["peak"], int(mag.max()))
                report[name]["at_full_scale"] += int(np.count_nonzero(mag == 32767))
        rest.append(limited.mix()[1])
    rest = np.concatenate(rest)                                     # [3 A, 2], limited.bus_delay() samples late
    report["delay"] = limited.bus_delay()[0]
    report["rest_level_quiet"] = rms(rest[int(0.4 * AUDIO):int(1.0 * AUDIO)])
    report["rest_level_talking"] = rms(rest[int((TALK[0] + 0.2) * AUDIO):int((TALK[1] - 0.1) * AUDIO)])
    report["tower_channels"], report["buses"] = tower_channels, [b.name for b in buses]
    return report


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--stations", type=int, default=12)
    ap.add_argument("--small", action="store_true", help="40 channels in 1 MHz, 6 stations")
    a = ap.parse_args()
    t0 = time.perf_counter()
    r = run(**SMALL) if a.small else run(a.channels, a.rate, a.stations)
    print("four stations at once on the tower bus (channels %s)" % r["tower_channels"])
    for name, what in (("plain", "without a limiter"), ("limited", "with Limiter()")):
        print("%-18s int16 peak %5d, %d samples at +-32767" % (what + ":", r[name]["peak"], r[name]["at_full_scale"]))
    print("everything else: level %.4f while the tower is quiet, %.4f while it talks (%.1f dB), %d samples late"
          % (r["rest_level_quiet"], r["rest_level_talking"],
             20.0 * np.log10(r["rest_level_talking"] / r["rest_level_quiet"]), r["delay"]))
    print("%.2f s wall" % (time.perf_counter() - t0))
