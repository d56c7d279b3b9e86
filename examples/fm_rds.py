#!/usr/bin/env python3
"""Naming the stations of a band: three broadcast WBFM stations with RDS in a synthetic 2.4 MSPS buffer, no SDR or sound
card.

`Tuner.run_all` gives the audio as always.  One more call, `Tuner.subcarrier`, taps the 57 kHz subcarrier of every
station's FM multiplex -- mixed down, low-pass filtered and decimated to 9 600 complex samples per station on the device --
and `radiocore.tools.rds` turns each of those into bits, groups, the PI code and the programme service name on the host.

    python examples/fm_rds.py
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import WBFM, Subcarrier, Tuner  # noqa: E402
from radiocore.tools import rds  # noqa: E402

RATE = 2_400_000        # wideband samples per second
CHANNEL = 240_000       # channel bandwidth (Hz)
AUDIO = 48_000
TAP_RATE = 9_600        # RDS baseband samples per second and station
STATIONS = ((99_300_000.0, 0x1234, "HIP FM  "), (100_100_000.0, 0xC0DE, "GFX 950 "), (100_850_000.0, 0x0B5E, "WAVE  64"))
LEVELS = (0.3, 0.1, 0.06)


def rds_signal(pi, ps, rate, delay):
    """One second of the RDS baseband at `rate` samples/s: type-0A groups cycling the name's four segments, differential
    and biphase coding, raised-cosine chips at rds.CHIP_RATE."""
    data = []
    for k in range(rds.CHIP_RATE // 2 // 104 + 2):
        seg = k % 4
        words = (pi, (1 << 10) | (10 << 5) | (1 << 3) | seg, 0xE210 + seg, (ord(ps[2 * seg]) << 8) | ord(ps[2 * seg + 1]))
        for info, name in zip(words, "ABCD"):
            word = (info << 10) | rds.checkword(info, rds.OFFSETS[name])
            data += [(word >> (25 - b)) & 1 for b in range(26)]
    e = np.bitwise_xor.accumulate(np.array(data, np.uint8)).astype(np.float64) * 2 - 1
    chip = np.concatenate([[0.0], np.stack([e, -e], axis=1).reshape(-1), [0.0, 0.0]])
    u = np.arange(rate) * (rds.CHIP_RATE / rate) - 0.5 - delay
    k = np.floor(u).astype(np.int64)
    w = 0.5 * (1 + np.cos(np.pi * (u - k)))
    k = np.clip(k, -1, len(chip) - 3)
    return chip[k + 1] * w + chip[k + 2] * (1 - w)


def station(i, pi, ps):
    """complex128 [CHANNEL]: stereo programme, 19 kHz pilot and RDS on 57 kHz, 75 kHz peak deviation."""
    rng = np.random.default_rng(700 + i)
    t = np.arange(CHANNEL) / CHANNEL
    left = 0.4 * np.sin(2 * np.pi * (440 + 110 * i) * t) + 0.3 * np.sin(2 * np.pi * 3000 * t + rng.uniform(0, 6))
    right = 0.4 * np.sin(2 * np.pi * (660 + 70 * i) * t) + 0.3 * np.sin(2 * np.pi * 5000 * t + rng.uniform(0, 6))
    th = 2 * np.pi * 19000 * t
    mpx = 0.9 * 0.85 * (0.5 * (left + right) + 0.5 * (left - right) * np.sin(2 * th)) + 0.09 * np.sin(th) \
        + 0.04 * rds_signal(pi, ps, CHANNEL, 0.1 + 0.3 * i) * np.sin(3 * th + 0.3)
    step = 2 * 75000 / CHANNEL * mpx                                       # phase step / pi
    step += (2 * np.round(step.sum() / 2) - step.sum()) / CHANNEL          # the phase closes on itself at the buffer's end
    return np.exp(1j * np.pi * np.cumsum(step))


def band(f_in):
    X = np.zeros(RATE, np.complex128)
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    for i, ((fc, pi, ps), level) in enumerate(zip(STATIONS, LEVELS)):
        X[(kk + int(fc - f_in)) % RATE] += np.fft.fft(station(i, pi, ps)) * (level * RATE / CHANNEL)
    rng = np.random.default_rng(57)
    x = np.fft.ifft(X) + 1e-3 * (rng.standard_normal(RATE) + 1j * rng.standard_normal(RATE))
    return x.astype(np.complex64)


def run():
    """Returns (audio [3, AUDIO, 2], [(PI, PS, groups found)] per station)."""
    tuner = Tuner(cuda=True)
    for fc, _, _ in STATIONS:
        tuner.add_channel(fc, CHANNEL, WBFM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(RATE))
    tuner.load(band(tuner.input_frequency))
    audio = tuner.run_all()
    tap = Subcarrier(CHANNEL, TAP_RATE, 57000, rds.taps(CHANNEL, TAP_RATE), cuda=True)
    y = tuner.subcarrier(tap)                       # complex64 [3, TAP_RATE]: all stations in one call
    found = []
    for row in y:
        g = rds.groups(rds.bits(row, TAP_RATE))
        found.append(rds.station(g) + (len(g),))
    return audio, found


if __name__ == "__main__":
    t0 = time.perf_counter()
    audio, found = run()
    for (fc, pi, ps), (got_pi, got_ps, n) in zip(STATIONS, found):
        print("%.2f MHz: PI %s  PS %r  (%d groups)%s" % (fc / 1e6, "%04X" % got_pi if got_pi is not None else "----", got_ps, n,
                                                        "" if (got_pi, got_ps) == (pi, ps) else "  MISMATCH"))
    print("audio %s, %.2f s wall" % (audio.shape, time.perf_counter() - t0))
