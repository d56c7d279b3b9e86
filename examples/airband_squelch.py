#!/usr/bin/env python3
"""A squelched band monitor: VHF airband (760 channels of 25 kHz) with a dozen stations on the air, no SDR or sound card.

Most channels of a band monitor are empty, and AM normalises every channel by its own level: without a squelch an
empty channel comes out as full-scale noise and the publisher sends all 760 of them.  Here the Tuner measures every
channel's level from the spectrum it already holds (`Tuner.levels()`), one calibration pass puts the thresholds 10 dB
over the noise floor (`squelch.threshold_over_floor`), and from then on `run_all()` mutes what is below its threshold
on the device and `open_mask()` tells `wire.frames` which channels to publish.

    python examples/airband_squelch.py [--channels 760] [--rate 20000000] [--seconds 3] [--stations 12]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AM, Tuner  # noqa: E402
from radiocore.tools import squelch, wire  # noqa: E402

CHANNEL = 25_000       # channel raster and bandwidth (Hz)
AUDIO = 8_000          # audio rate (Hz)
OVER_FLOOR_DB = 10.0


def band(rate, centres, f_in, on_air, rng):
    """One second of complex baseband at `rate` samples/s: an AM station (one voice-band tone) on each channel of
    `on_air`, at levels up to 20 dB apart, and receiver noise everywhere."""
    n = int(rate)
    X = np.zeros(n, np.complex128)
    t = np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    for i in on_air:
        level = 10.0 ** rng.uniform(-1.0, 0.0)
        tone = 300.0 + (37.0 * i) % 3000.0
        s = level * (1 + rng.uniform(0.3, 0.8) * np.sin(2 * np.pi * tone * t)) * np.exp(2j * np.pi * int(rng.integers(-1000, 1001)) * t)
        X[(kk + int(centres[i] - f_in)) % n] += np.fft.fft(s) * (n / CHANNEL)
    x = np.fft.ifft(X)
    x += 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def run(channels=760, rate=20_000_000, seconds=3, stations=12, publish=None):
    """Returns (opened, planted, messages): per second after the calibration pass the channel indices the squelch
    opened and the ones that were on the air, and every published (frequency, float32 [A, 1])."""
    first = 118_012_500.0                          # the centre of the first 25 kHz airband channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    rng = np.random.default_rng(121)
    opened, planted, out = [], [], []
    for second in range(seconds):
        # stations come and go from second to second
        on_air = sorted(int(i) for i in rng.choice(channels, stations, replace=False))
        tuner.load(band(rate, centres, tuner.input_frequency, on_air, rng))
        if second == 0:
            # calibration: the median power density over the channels is the floor, whoever is on the air meanwhile
            thresholds = squelch.threshold_over_floor(tuner.levels(), CHANNEL, OVER_FLOOR_DB)
            tuner.set_squelch(thresholds)
            continue
        audio = tuner.run_all()                    # [C, A, 1]: closed channels are exact zeros
        mask = tuner.open_mask()
        for message in wire.frames(tuner.channels(), audio, open_mask=mask):
            if publish is not None:
                publish(message)                   # socket.send_multipart(message) in a server
            out.append(wire.parse_frame(message, 1))
        opened.append([int(i) for i in np.flatnonzero(mask)])
        planted.append(on_air)
    return opened, planted, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=int, default=3)
    ap.add_argument("--stations", type=int, default=12)
    a = ap.parse_args()
    t0 = time.perf_counter()
    opened, planted, msgs = run(a.channels, a.rate, a.seconds, a.stations)
    for k, (o, p) in enumerate(zip(opened, planted)):
        print("second %d: open %s  (on the air: %s)%s" % (k + 1, o, p, "" if o == p else "  MISMATCH"))
    print("%d frames published instead of %d, %.2f s wall" % (len(msgs), a.channels * len(opened), time.perf_counter() - t0))
