#!/usr/bin/env python3
"""A band scan and a squelch over a noise floor that is not flat.  No SDR or sound card.

The band is the airband of examples/band_scan.py -- 760 channels of 25 kHz -- but behind a front end whose noise rises by
20 dB from the lower band edge to the upper one, and the stations are weak: 13 .. 17 dB over the noise of their own channel.
The scan of examples/band_scan.py takes the median cell of the whole band as the floor: at 10 dB over it the stations in the
quiet lower part of the band are missed, and a threshold low enough to find them marks the noisy upper part as occupied.

`Tuner.set_floor(NoiseFloor(...))` tracks the floor around every cell on the device, buffer after buffer (OS-CFAR: the
lower quartile of the 62 cells around a cell, the cell's neighbours left out).  `spectrum.occupied(power, 10, floor=...)`
then finds every station and nothing else, and `set_squelch(OverFloor(10))` opens exactly their channels -- without the
calibration pass of examples/airband_squelch.py, and following the floor when it moves.

    python examples/band_scan_cfar.py [--small] [--channels 760] [--rate 20000000] [--stations 12] [--seconds 3]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), HERE]

import numpy as np  # noqa: E402

from radiocore import AM, NoiseFloor, OverFloor, Tuner  # noqa: E402
from radiocore.tools import spectrum  # noqa: E402

CHANNEL = 25_000          # channel raster and bandwidth (Hz); the scan's cells are as wide, and the raster puts them on the channels
AUDIO = 8_000
FIRST = 118_012_500.0     # the centre of the first 25 kHz airband channel
TILT_DB = 20.0            # the noise density rises by this much across the buffer's band
OVER_FLOOR_DB = 10.0
LOW_DB = 5.0              # what the global median needs to find the weakest station in the quietest part
SMALL = dict(channels=120, rate=4_000_000, stations=7, seconds=3)      # a geometry that runs in a few seconds


def band(rate, centres, f_in, on_air, rng, noise=1e-4):
    """One second of complex baseband at `rate` samples/s: receiver noise whose density is tilted by TILT_DB across the
    band (`noise`: its standard deviation per component at the band's centre), and on each channel of `on_air`
    ({channel: dB over the noise its channel holds}) an AM station with one voice-band tone."""
    n = int(rate)
    s = np.fft.fftfreq(n, 1.0 / n)                                              # signed bin of every fft bin
    density = 2.0 * noise ** 2 / n * 10.0 ** (TILT_DB / 10.0 * s / n)           # power per bin
    X = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(density / 2.0) * n
    t = np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    for i, db in on_air.items():
        centre = int(centres[i] - f_in)
        m = rng.uniform(0.3, 0.8)
        floor = 2.0 * noise ** 2 / n * 10.0 ** (TILT_DB / 10.0 * centre / n) * CHANNEL
        a = np.sqrt(floor * 10.0 ** (db / 10.0) / (1.0 + m * m / 2.0))
        tone = 300.0 + (37.0 * i) % 3000.0
        st = a * (1 + m * np.sin(2 * np.pi * tone * t)) * np.exp(2j * np.pi * int(rng.integers(-1000, 1001)) * t)
        X[(kk + centre) % n] += np.fft.fft(st) * (n / CHANNEL)
    return np.fft.ifft(X).astype(np.complex64)


def channels_of(runs, n, cells, channels, f_in):
    """The channels the runs of `spectrum.occupied` lie in (every cell of a run; None outside every channel), ascending."""
    lower = FIRST - CHANNEL / 2
    f = spectrum.cell_frequencies(f_in, -(n // 2), n, cells)
    out = set()
    for a, b, _ in runs:
        for c in range(a, b + 1):
            i = int((f[c] - lower) // CHANNEL)
            out.add(i if 0 <= i < channels else None)
    return sorted(out, key=lambda i: (i is None, i))


def run(channels=760, rate=20_000_000, stations=12, seconds=3):
    """Per second: the channels on the air, what the global-median scan finds at OVER_FLOOR_DB and at LOW_DB, what the CFAR
    scan finds at OVER_FLOOR_DB, and what `set_squelch(OverFloor(OVER_FLOOR_DB))` opens -- lists of channel indices."""
    centres = [FIRST + CHANNEL * i for i in range(channels)]
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    n = int(rate)
    cells = n // CHANNEL
    tuner.set_floor(NoiseFloor(CHANNEL, half=32, guard=1, quantile=0.25))
    tuner.set_squelch(OverFloor(OVER_FLOOR_DB))                 # no calibration pass: the first buffer is gated already
    rng = np.random.default_rng(121)
    out = []
    for second in range(seconds):
        # stations come and go; the weakest sits in the quiet lowest tenth of the band
        picks = [int(rng.integers(0, max(channels // 10, 1)))] + [int(i) for i in rng.choice(channels, stations - 1, replace=False)]
        on_air = {i: float(rng.uniform(13.0, 17.0)) for i in picks}
        on_air[picks[0]] = 13.0
        # the whole floor moves as well: 3 dB down in the second buffer
        tuner.load(band(rate, centres, tuner.input_frequency, on_air, rng, noise=1e-4 * (0.7 if second == 1 else 1.0)))
        power = tuner.power_spectrum(cells)
        f_in = tuner.input_frequency
        median_hi = channels_of(spectrum.occupied(power, OVER_FLOOR_DB), n, cells, channels, f_in)
        median_lo = channels_of(spectrum.occupied(power, LOW_DB), n, cells, channels, f_in)
        cfar = channels_of(spectrum.occupied(power, OVER_FLOOR_DB, floor=tuner.floor()), n, cells, channels, f_in)
        audio = tuner.run_all()                                 # [C, A, 1]: closed channels are exact zeros
        mask = tuner.open_mask()
        assert not audio[~mask].any()
        out.append(dict(on_air=sorted(on_air), median=median_hi, median_low=median_lo, cfar=cfar,
                        opened=[int(i) for i in np.flatnonzero(mask)]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="%(channels)d channels in %(rate)d samples, %(stations)d stations" % SMALL)
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--stations", type=int, default=12)
    ap.add_argument("--seconds", type=int, default=3)
    a = ap.parse_args()
    geometry = SMALL if a.small else dict(channels=a.channels, rate=a.rate, stations=a.stations, seconds=a.seconds)
    t0 = time.perf_counter()
    for k, r in enumerate(run(**geometry)):
        air = r["on_air"]
        print("second %d: on the air %s" % (k, air))
        print("  global median, %4.1f dB: missed %s, empty %s" % (OVER_FLOOR_DB, sorted(set(air) - set(r["median"])), sorted(set(r["median"]) - set(air), key=str)))
        print("  global median, %4.1f dB: missed %s, empty channels marked: %d" % (LOW_DB, sorted(set(air) - set(r["median_low"])), len(set(r["median_low"]) - set(air))))
        print("  CFAR scan,     %4.1f dB: %s%s" % (OVER_FLOOR_DB, r["cfar"], "" if r["cfar"] == air else "  MISMATCH"))
        print("  squelch OverFloor(%g): open %s%s" % (OVER_FLOOR_DB, r["opened"], "" if r["opened"] == air else "  MISMATCH"))
    print("%.2f s wall" % (time.perf_counter() - t0))
