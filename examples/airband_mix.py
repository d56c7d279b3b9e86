#!/usr/bin/env python3
"""A band monitor one can listen to: VHF airband (760 channels of 25 kHz) mixed down to three stereo streams on the device,
no SDR or sound card.

760 audio rows can be recorded; nobody can listen to them.  `Tuner.set_mix` adds the channels the frame gate left open into
a few buses, every channel at its own gain and place between left and right, in one fixed order, and
`run_all_packed(..., buses=True)` packs and drains the bus rows instead of the channel rows: a "tower group" of a few
channels panned by frequency, "everything else" 6 dB down in the middle, and a standby bus of channels nobody uses, which
never produces a frame.  The stations are those of examples/airband_gate.py, keying on and off over three buffers.  Every
drained payload is compared with the numpy quantisation of the definition's mix (include/rcfm.h, "audio buses") of the
audio `run_all` gives for the same buffers, and the bytes drained for the buses are set against the bytes the open channel
rows would have taken.

    python examples/airband_mix.py [--channels 760] [--rate 20000000] [--stations 12] [--small]
"""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AM, PCM, Bus, Drain, FrameGate, Mixer, Tuner  # noqa: E402
from radiocore.tools import squelch  # noqa: E402

_spec = importlib.util.spec_from_file_location("airband_gate", os.path.join(ROOT, "examples", "airband_gate.py"))
airband_gate = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(airband_gate)

CHANNEL, AUDIO, SECONDS, FRAMES = airband_gate.CHANNEL, airband_gate.AUDIO, airband_gate.SECONDS, airband_gate.FRAMES
OVER_FLOOR_DB = airband_gate.OVER_FLOOR_DB
SMALL = dict(channels=40, rate=1_000_000, stations=6)
TOWER, STANDBY = 4, 3          # channels of the tower group (stations) and of the standby bus (no station)
GAIN = 8192.0                  # int16 per unit of audio: four AM stations at once stay inside 16 bits


def bus_model(audio, mask, bus):
    """[A, 2] float32: the definition's stereo mix of mono audio [C, A, 1] for one bus -- segments of 16 routes, each summed
    from +0 over its open routes in order, the segment sums added from +0 in order; float32 products and sums."""
    A = audio.shape[1]
    acc = np.zeros((A, 2), np.float32)
    for s0 in range(0, len(bus), 16):
        s = np.zeros((A, 2), np.float32)
        for c, (gl, gr) in zip(bus.channels[s0:s0 + 16], bus.gains[s0:s0 + 16]):
            if mask[c]:
                s = s + np.stack([gl * audio[c, :, 0], gr * audio[c, :, 0]], axis=-1)
        acc = acc + s
    return acc


def quantise(x, gain):
    """PCM("int16", gain) in numpy: one float32 product, round to nearest even, clamp to +-32767."""
    return np.rint(np.clip(np.asarray(x, np.float32) * np.float32(gain), -32767.0, 32767.0)).astype(np.int16)


def run(channels=760, rate=20_000_000, stations=12):
    """Three buffers through a mixing tuner and, for the comparison, through one that returns the channel audio.  Returns
    the buses and one dict per second: which buses were drained, whether every payload equalled the model's, and the bytes
    drained for the buses and for the open channel rows."""
    first = 118_012_500.0                          # the centre of the first 25 kHz airband channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuners = []
    for _ in range(2):
        tuner = Tuner(cuda=True)
        for f in centres:
            tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
        tuner.request_bandwidth(float(rate))
        tuners.append(tuner)
    mixing, plain = tuners
    rng = np.random.default_rng(122)
    on_air = airband_gate.transmissions(channels, stations, rng)
    # the buses: a few stations as the tower group, left to right by frequency; channels nobody uses on standby; the rest
    tower_channels = sorted(on_air)[:TOWER]
    standby_channels = [c for c in range(channels) if c not in on_air][:STANDBY]
    others = [c for c in range(channels) if c not in tower_channels and c not in standby_channels]
    buses = [Bus.of(tower_channels, gain_db=0.0, pan=np.linspace(-0.7, 0.7, len(tower_channels)), name="tower"),
             Bus.of(others, gain_db=-6.0, pan=0.0, name="everything else"),
             Bus.of(standby_channels, gain_db=0.0, pan=0.0, name="standby")]
    mixing.set_mix(Mixer(buses, stereo=True))
    gate = FrameGate(frames=FRAMES, hang=0.25, lead=1, ramp=0.005)
    pcm = PCM("int16", GAIN)
    drain = Drain(len(buses), (AUDIO, 2), pcm.dtype, depth=2)
    seconds = []
    for second in range(SECONDS):
        x = airband_gate.band(rate, centres, mixing.input_frequency, on_air, second, rng)
        mixing.load(x)
        plain.load(x)
        if second == 0:
            thresholds = squelch.threshold_over_floor(plain.levels(), CHANNEL, OVER_FLOOR_DB)
            for t in tuners:
                t.set_gate(gate, open=thresholds)
        mixing.run_all_packed(pcm, drain=drain, buses=True)
        audio = plain.run_all()                                  # [C, A, 1]: the same launches, the same gate states
        mask = plain.open_mask()
        with drain.next() as (index, rows):
            drained = [int(m) for m in index]
            equal = all(np.array_equal(rows[k], quantise(bus_model(audio, mask, buses[m]), GAIN)) for k, m in enumerate(drained))
            bus_bytes = int(rows.nbytes)
        idle = [m for m, b in enumerate(buses) if not mask[b.channels].any()]
        seconds.append({"drained": drained, "idle": idle, "equal": equal, "active": mixing.mix_active().tolist(),
                        "open_channels": int(mask.sum()), "bus_bytes": bus_bytes,
                        "channel_bytes": int(mask.sum()) * AUDIO * pcm.dtype.itemsize})
    drain.close()
    return buses, seconds


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--stations", type=int, default=12)
    ap.add_argument("--small", action="store_true", help="40 channels in 1 MHz, 6 stations")
    a = ap.parse_args()
    t0 = time.perf_counter()
    buses, seconds = run(**SMALL) if a.small else run(a.channels, a.rate, a.stations)
    for s, r in enumerate(seconds):
        names = ", ".join("%s (%d open)" % (buses[m].name, r["active"][m]) for m in r["drained"]) or "nothing"
        print("second %d: drained %s; payloads %s the model's; %d bytes for the buses, %d for the %d open channel rows"
              % (s, names, "equal" if r["equal"] else "DIFFER FROM", r["bus_bytes"], r["channel_bytes"], r["open_channels"]))
    print("%.2f s wall" % (time.perf_counter() - t0))
