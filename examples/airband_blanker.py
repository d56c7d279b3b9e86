#!/usr/bin/env python3
"""Impulse noise on a band monitor: the VHF airband buffer of airband_squelch.py with ignition pulses on it, no SDR or sound
card.

A pulse of three samples is white across the whole band: after `Tuner.load` it sits in every one of the 760 channels, as
full-scale clicks in the AM audio (whose tail normalises by the buffer's own level) and as a lift of `levels()` in the empty
channels, towards the squelch threshold.  `Tuner.set_blanker(NoiseBlanker())` takes the pulses out of the time-domain buffer
ahead of the FFT, where they are still three samples long.  Printed per station on the air: the audio error against the
pulse-free buffer without and with the blanker; then what the blanker did, how many empty channels each case lifts over
a squelch threshold calibrated on the clean band, and by how much (the median over the empty channels).  Blanking is not
free: every zeroed sample of a strong station is a small wideband click of its own, so on a band whose floor lies 80 dB
under its stations the empty channels stay above the clean floor -- far less than under the pulses.

    python examples/airband_blanker.py [--channels 760] [--rate 20000000] [--stations 12] [--pulses 200]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), os.path.join(ROOT, "examples")]

import numpy as np  # noqa: E402

from airband_squelch import AUDIO, CHANNEL, band  # noqa: E402

OVER_RMS_DB = 35.0     # an ignition pulse over the buffer's RMS
PULSE = 3              # samples
OVER_FLOOR_DB = 6.0    # the squelch threshold over the clean band's floor


def add_pulses(x, count, rng):
    """x with `count` pulses of PULSE samples at random places, OVER_RMS_DB over its RMS, at random phases."""
    y = x.copy()
    amp = 10.0 ** (OVER_RMS_DB / 20.0) * float(np.sqrt(np.mean(np.abs(x) ** 2)))
    for q in rng.choice(x.shape[0] - PULSE, count, replace=False):
        y[q:q + PULSE] += (amp * np.exp(2j * np.pi * rng.uniform(size=PULSE))).astype(np.complex64)
    return y


def buffers(channels=760, rate=20_000_000, stations=12, pulses=200, seed=121):
    """(clean, dirty, centres, input frequency, on_air): one second of the airband with `stations` on the air, without and
    with the pulses."""
    first = 118_012_500.0
    centres = [first + CHANNEL * i for i in range(channels)]
    f_in = (centres[0] + centres[-1]) / 2.0
    rng = np.random.default_rng(seed)
    on_air = sorted(int(i) for i in rng.choice(channels, stations, replace=False))
    clean = band(rate, centres, f_in, on_air, rng)
    return clean, add_pulses(clean, pulses, rng), centres, f_in, on_air


def envelope(x, offset):
    """|channel| of the 25 kHz channel `offset` Hz above the buffer's centre, on the host: the bins around it, brought down."""
    n = x.shape[0]
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    X = np.fft.fft(x.astype(np.complex128))
    return np.abs(np.fft.ifft(X[(kk + int(offset)) % n])) * (CHANNEL / n)


def envelope_errors(x, clean, centres, f_in, on_air):
    """Per station: rms(|channel of x| - |channel of clean|) / mean |channel of clean|."""
    out = []
    for i in on_air:
        e, e0 = envelope(x, centres[i] - f_in), envelope(clean, centres[i] - f_in)
        out.append(float(np.sqrt(np.mean((e - e0) ** 2)) / np.mean(e0)))
    return out


def run(channels=760, rate=20_000_000, stations=12, pulses=200, blanker=None):
    """On the device.  Returns (on_air, error without the blanker, error with it, blanker_stats, lifted without, lifted
    with, lift in dB without, with): the errors are rms(audio - audio of the clean buffer) per station on the air, `lifted`
    counts the empty channels whose level exceeds the threshold, and the lift is the median level of the empty channels over
    their median level in the clean buffer."""
    from radiocore import AM, NoiseBlanker, Tuner
    from radiocore.tools import squelch
    clean, dirty, centres, f_in, on_air = buffers(channels, rate, stations, pulses)
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    tuner.load(clean)
    floor = tuner.levels()
    thresholds = squelch.threshold_over_floor(floor, CHANNEL, OVER_FLOOR_DB)
    want = tuner.run_all()[on_air, :, 0]
    empty = np.setdiff1d(np.arange(channels), on_air)
    errors, lifted, lift_db = [], [], []
    for nb in (None, blanker if blanker is not None else NoiseBlanker()):
        tuner.set_blanker(nb)
        tuner.load(dirty)
        levels = tuner.levels()
        lifted.append(int(np.sum(levels[empty] > thresholds[empty])))
        lift_db.append(float(10.0 * np.log10(np.median(levels[empty]) / np.median(floor[empty]))))
        got = tuner.run_all()[on_air, :, 0]
        errors.append([float(np.sqrt(np.mean((g - w) ** 2))) for g, w in zip(got, want)])
    return on_air, errors[0], errors[1], tuner.blanker_stats(), lifted[0], lifted[1], lift_db[0], lift_db[1]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--stations", type=int, default=12)
    ap.add_argument("--pulses", type=int, default=200)
    a = ap.parse_args()
    on_air, before, after, stats, lifted0, lifted1, lift0, lift1 = run(a.channels, a.rate, a.stations, a.pulses)
    for i, b, c in zip(on_air, before, after):
        print("channel %3d: audio error %.4f without the blanker, %.4f with it" % (i, b, c))
    print("blanker: %d hits, %d samples blanked (%.3f %% of the buffer)" % (stats[0], stats[1], 100.0 * stats[1] / a.rate))
    print("empty channels over the squelch threshold: %d without the blanker, %d with it" % (lifted0, lifted1))
    print("median level of the empty channels over the clean floor: %.1f dB without the blanker, %.1f dB with it" % (lift0, lift1))
