#!/usr/bin/env python3
"""Image rejection for an 8-bit receiver: the squelched airband monitor of airband_squelch.py behind an RTL-SDR, no SDR needed.

The receivers that deliver uint8 IQ are the ones whose I and Q paths do not match: 5 % gain and 3 degrees phase error put
an image of every station at the mirrored frequency, 29 dB down, and a DC offset sits on the tuning frequency.  For a
squelched band monitor the image of every strong station opens the squelch of the mirror channel.  Here the airband
buffer goes through that receiver model (`iq.impair`), is quantised to cu8 and loaded as it is (`Tuner.load_raw`), once
into a tuner with `set_iq_balance("auto", dc_notch=1)` -- beta is estimated from each buffer's own spectrum and the image
removed before any channel is read -- and once into a tuner without it, both gated by the same thresholds.

    python examples/rtl_image_reject.py [--channels 760] [--rate 20000000] [--seconds 3] [--stations 12]
"""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AM, Tuner  # noqa: E402
from radiocore.tools import iq, squelch  # noqa: E402

_spec = importlib.util.spec_from_file_location("airband_squelch", os.path.join(ROOT, "examples", "airband_squelch.py"))
airband = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(airband)

CHANNEL, AUDIO, OVER_FLOOR_DB = airband.CHANNEL, airband.AUDIO, airband.OVER_FLOOR_DB
GAIN, PHASE = 1.05, np.deg2rad(3.0)      # the receiver's Q path against its I path
DC = 0.02 + 0.01j                        # ... and its DC offset, in full scales
STRONG_DB = 6.0                          # a station this far below the strongest still shows its image over the thresholds


def receive(x, rng):
    """uint8 [n, 2]: the true baseband x as an RTL-SDR delivers it.  The gain is set so that the strongest peak uses 90 % of
    full scale; the receiver's own noise, half an LSB per component, dithers the 8-bit quantiser."""
    y = iq.impair(x, GAIN, PHASE)
    y *= 0.9 / max(np.abs(y.real).max(), np.abs(y.imag).max())
    y += DC + (0.5 / 128.0) * (rng.standard_normal(y.shape[0]) + 1j * rng.standard_normal(y.shape[0]))
    v = np.stack([y.real, y.imag], axis=-1) * 128.0 + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def monitor(centres, rate, balance):
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    if balance:
        tuner.set_iq_balance("auto", dc_notch=1)
    return tuner


def run(channels=760, rate=20_000_000, seconds=3, stations=12):
    """Per second after the calibration pass: (the channels the balanced monitor opened, the ones the unbalanced monitor
    opened, the ones on the air, the mirror channels of the strong stations that are not on the air themselves)."""
    first = 118_012_500.0
    centres = [first + CHANNEL * i for i in range(channels)]
    clean, plain = monitor(centres, rate, True), monitor(centres, rate, False)
    rng = np.random.default_rng(121)
    balanced, unbalanced, planted, ghosts = [], [], [], []
    for second in range(seconds):
        on_air = sorted(int(i) for i in rng.choice(channels, stations, replace=False))
        raw = receive(airband.band(rate, centres, clean.input_frequency, on_air, rng), rng)
        clean.load_raw(raw)
        plain.load_raw(raw)
        if second == 0:
            # calibration on the clean band: the floor is the receiver's noise, not somebody's image
            thresholds = squelch.threshold_over_floor(clean.levels(), CHANNEL, OVER_FLOOR_DB)
            clean.set_squelch(thresholds)
            plain.set_squelch(thresholds)
            continue
        clean.run_all()
        plain.run_all()
        levels = clean.levels()
        strong = [i for i in on_air if levels[i] >= levels[on_air].max() * 10.0 ** (-STRONG_DB / 10.0)]
        balanced.append([int(i) for i in np.flatnonzero(clean.open_mask())])
        unbalanced.append([int(i) for i in np.flatnonzero(plain.open_mask())])
        planted.append(on_air)
        # the channels lie symmetrically about the input frequency: the mirror of channel i is channel C - 1 - i
        ghosts.append(sorted(channels - 1 - i for i in strong if channels - 1 - i not in on_air))
    return balanced, unbalanced, planted, ghosts


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=int, default=3)
    ap.add_argument("--stations", type=int, default=12)
    a = ap.parse_args()
    t0 = time.perf_counter()
    for k, (b, u, p, g) in enumerate(zip(*run(a.channels, a.rate, a.seconds, a.stations))):
        print("second %d: on the air %s" % (k + 1, p))
        print("  with set_iq_balance(\"auto\", dc_notch=1): open %s%s" % (b, "" if b == p else "  MISMATCH"))
        print("  without: open %s  (mirrors of the strong stations: %s)" % (u, g))
    print("%.2f s wall" % (time.perf_counter() - t0))
