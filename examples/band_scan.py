#!/usr/bin/env python3
"""A band scan: where are the stations, before any channel is tuned?  No SDR or sound card.

The buffer is the one of examples/airband_squelch.py: VHF airband, 760 channels of 25 kHz, a dozen AM stations on the
air.  The Tuner holds the buffer's spectrum after `load`; one `Tuner.power_spectrum` call bins all of it into cells of
6.25 kHz (four per channel: a carrier and its voice sidebands fill the middle two), `spectrum.occupied` keeps the runs of
cells 10 dB over the floor (the median cell), and each run is the channel whose band contains its strongest cell.

    python examples/band_scan.py [--small] [--channels 760] [--rate 20000000] [--stations 12]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), HERE]

import numpy as np  # noqa: E402

from airband_squelch import CHANNEL, band  # noqa: E402
from radiocore import Tuner  # noqa: E402
from radiocore.tools import spectrum  # noqa: E402

CELL = 6250               # cell width (Hz): a quarter of a channel
OVER_FLOOR_DB = 10.0      # a cell is occupied from 10 dB over the median cell
FIRST = 118_012_500.0     # the centre of the first 25 kHz airband channel
SMALL = dict(channels=120, rate=4_000_000, stations=7)      # a geometry that runs in a few seconds


def channels_of(runs, n, cells, channels, f_in=None):
    """The channel index of each run of `occupied`: the channel whose band contains the run's strongest cell (None
    outside every channel), in ascending order.  n: samples of the buffer, cells: of the full-span spectrum."""
    lower = FIRST - CHANNEL / 2
    f_in = lower + channels * CHANNEL / 2 if f_in is None else f_in      # the Tuner centres the band on its channels
    f = spectrum.cell_frequencies(f_in, -(n // 2), n, cells)
    out = []
    for _, _, strongest in runs:
        i = int((f[strongest] - lower) // CHANNEL)
        out.append(i if 0 <= i < channels else None)
    return sorted(out, key=lambda i: (i is None, i))


def run(channels=760, rate=20_000_000, stations=12):
    """Returns (found, planted, runs, x, input_frequency): the channels the scan found and the ones that were on the
    air, both ascending, the occupied runs of cells, and the buffer itself."""
    centres = [FIRST + CHANNEL * i for i in range(channels)]
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, None)         # the scan needs no demodulator
    tuner.request_bandwidth(float(rate))
    rng = np.random.default_rng(121)
    planted = sorted(int(i) for i in rng.choice(channels, stations, replace=False))
    x = band(rate, centres, tuner.input_frequency, planted, rng)
    tuner.load(x)
    n = int(rate)
    cells = n // CELL
    power = tuner.power_spectrum(cells)             # the whole band, one call, float32 [cells]
    runs = spectrum.occupied(power, OVER_FLOOR_DB)
    return channels_of(runs, n, cells, channels, tuner.input_frequency), planted, runs, x, tuner.input_frequency


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="%(channels)d channels in %(rate)d samples, %(stations)d stations" % SMALL)
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--stations", type=int, default=12)
    a = ap.parse_args()
    geometry = SMALL if a.small else dict(channels=a.channels, rate=a.rate, stations=a.stations)
    t0 = time.perf_counter()
    found, planted, runs, _, f_in = run(**geometry)
    freq = spectrum.cell_frequencies(f_in, -(geometry["rate"] // 2), geometry["rate"], geometry["rate"] // CELL)
    for (a0, a1, top), ch in zip(runs, found):
        print("cells %5d..%-5d strongest at %.5f MHz -> channel %s (%.4f MHz)"
              % (a0, a1, freq[top] / 1e6, ch, (FIRST + CHANNEL * ch) / 1e6 if ch is not None else float("nan")))
    print("found    %s\non the air %s%s" % (found, planted, "" if found == planted else "  MISMATCH"))
    print("%.2f s wall" % (time.perf_counter() - t0))
