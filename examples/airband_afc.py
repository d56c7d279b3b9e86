#!/usr/bin/env python3
"""Frequency correction on a band monitor: VHF airband (760 channels of 25 kHz), a dozen stations off their channel
centres (8.33 kHz spacing, offset-carrier operation, tired crystals), no SDR or sound card.

The Tuner reads where inside its channel each station sits from the spectrum it already holds (`Tuner.carriers()`),
`afc.corrections` turns that into one step per channel -- nothing for the channels whose strongest bin is not well over
the noise floor -- and `Tuner.retune` moves the channels there without rebuilding anything: the same loaded buffer is
read again at once, now centred.

    python examples/airband_afc.py [--channels 760] [--rate 20000000] [--stations 12]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AM, Tuner  # noqa: E402
from radiocore.tools import afc  # noqa: E402

CHANNEL = 25_000       # channel raster and bandwidth (Hz)
AUDIO = 8_000          # audio rate (Hz)
OVER_FLOOR_DB = 20.0   # a carrier worth following: this far over the median bin of its channel's neighbourhood
MAX_STEP = 10_000      # Hz per pass


def band(rate, centres, f_in, on_air, offsets, rng):
    """One second of complex baseband at `rate` samples/s: an AM station (one voice-band tone) on each channel of
    `on_air`, offsets[j] Hz off its channel centre, at levels up to 20 dB apart, and receiver noise everywhere."""
    n = int(rate)
    X = np.zeros(n, np.complex128)
    t = np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    for i, off in zip(on_air, offsets):
        level = 10.0 ** rng.uniform(-1.0, 0.0)
        tone = 300.0 + (37.0 * i) % 3000.0
        s = level * (1 + rng.uniform(0.3, 0.8) * np.sin(2 * np.pi * tone * t)) * np.exp(2j * np.pi * int(off) * t)
        X[(kk + int(centres[i] - f_in)) % n] += np.fft.fft(s) * (n / CHANNEL)
    x = np.fft.ifft(X)
    x += 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def run(channels=760, rate=20_000_000, stations=12):
    """Returns (on_air, truth, measured, after): the channels on the air, the offsets they were given, the offsets the
    first carriers pass measured there, and what the second pass reads there after the retune."""
    first = 118_012_500.0                          # the centre of the first 25 kHz airband channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    rng = np.random.default_rng(121)
    on_air = sorted(int(i) for i in rng.choice(channels, stations, replace=False))
    truth = [int(v) for v in rng.choice([-8333, -5000, -2500, -1234, -7, 0, 415, 2500, 5000, 8333], stations)]
    tuner.load(band(rate, centres, tuner.input_frequency, on_air, truth, rng))
    peak_bin, peak_power, centroid, _ = tuner.carriers()
    # the floor: the median over the channels of the power per bin, levels() / bandwidth
    floor = float(np.median(tuner.levels())) / CHANNEL
    step = afc.corrections(peak_bin, peak_power, centroid, floor * 10.0 ** (OVER_FLOOR_DB / 10.0), MAX_STEP)
    moved = [int(i) for i in np.flatnonzero(step)]
    assert set(moved) <= set(on_air), "a channel without a station was moved"
    tuner.retune(step)                             # the loaded buffer stays: no second load
    after = tuner.carriers()[0]
    audio = tuner.run_all()                        # ... and the stations demodulate centred
    assert audio.shape == (channels, AUDIO, 1)
    return on_air, truth, [int(peak_bin[i]) for i in on_air], [int(after[i]) for i in on_air]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--stations", type=int, default=12)
    a = ap.parse_args()
    t0 = time.perf_counter()
    on_air, truth, measured, after = run(a.channels, a.rate, a.stations)
    for i, tr, me, af in zip(on_air, truth, measured, after):
        print("channel %3d: %+5d Hz off centre, measured %+5d Hz, after the retune %+d Hz%s"
              % (i, tr, me, af, "" if me == tr and af == 0 else "  MISMATCH"))
    print("%.2f s wall" % (time.perf_counter() - t0))
