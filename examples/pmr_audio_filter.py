#!/usr/bin/env python3
"""The voice filter behind a tone squelch: the stations of examples/pmr_tone_squelch.py, published without their hum.

The tone squelch opens a channel on its group's CTCSS tone -- and that tone, 88.5 Hz here, is then part of the audio.
Every receiver for these bands strips it with a 300 Hz high-pass, and de-emphasises narrow FM at 6 dB per octave.
`Tuner.set_audio_filter(VOICE_NFM)` queues both (and a 3 kHz low-pass) as five biquad sections per channel behind the
demodulators: behind the tone bank, which must still see the tone, and before the squelch zeroes the closed rows.  The
filter's state is carried from buffer to buffer, so nothing clicks at the buffer boundary.

    python examples/pmr_audio_filter.py [--channels 16] [--rate 1000000] [--seconds 2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), os.path.join(ROOT, "examples")]

import numpy as np  # noqa: E402

import pmr_tone_squelch as pmr  # noqa: E402
from radiocore import FM, ToneBank, Tuner  # noqa: E402
from radiocore.tools import tones  # noqa: E402
from radiocore.tools.audiofilter import VOICE_NFM  # noqa: E402


def hum_db(row, f_hz=pmr.WANTED):
    """Level of the row's component at f_hz in dB relative to full scale: a Hann-windowed projection over the buffer."""
    n = row.shape[0]
    k = np.arange(n)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * k / n)
    z = np.sum(w * row.astype(np.float64) * np.exp(-2j * np.pi * f_hz * k / n)) / np.sum(w)
    return 20.0 * np.log10(max(2.0 * abs(z), 1e-30))


def attenuation_db(filt, f_hz=pmr.WANTED, rate=pmr.AUDIO):
    """What the filter's sections take off a sinusoid of f_hz, in dB (positive)."""
    z = np.exp(-2j * np.pi * f_hz / rate)
    h = 1.0
    for b0, b1, b2, a0, a1, a2 in filt.sections(rate):
        h *= (b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)
    return -20.0 * np.log10(abs(h))


def run(channels=16, rate=1_000_000, seconds=2):
    """One (opened, {channel: (hum before, hum after)} in dB, filtered audio [C, A, 1]) per second."""
    centres = [446_006_250.0 + pmr.CHANNEL * i for i in range(channels)]
    tuners = []
    for voice in (None, VOICE_NFM):
        t = Tuner(cuda=True)
        for f in centres:
            t.add_channel(f, pmr.CHANNEL, FM(pmr.CHANNEL, pmr.AUDIO, cuda=True))
        t.request_bandwidth(float(rate))
        t.set_tones(ToneBank(tones.CTCSS), want=pmr.WANTED, ratio=pmr.RATIO)
        t.set_audio_filter(voice)
        tuners.append(t)
    rng = np.random.default_rng(446)
    out = []
    for second in range(seconds):
        where = sorted(int(i) for i in rng.choice(channels, 5, replace=False))
        other = rng.choice([f for f in tones.CTCSS if f != pmr.WANTED], 3, replace=False)
        on_air = dict(zip(where, [pmr.WANTED, float(other[0]), float(other[1]), pmr.WANTED, float(other[2])]))
        x = pmr.band(rate, centres, tuners[0].input_frequency, on_air, rng)
        audio, masks = [], []
        for t in tuners:
            t.load(x)
            audio.append(t.run_all())
            masks.append(t.open_mask())
        assert np.array_equal(masks[0], masks[1])          # the tone bank sees the unfiltered audio: the same channels open
        opened = [int(i) for i in np.flatnonzero(masks[1])]
        out.append((opened, {c: (hum_db(audio[0][c, :, 0]), hum_db(audio[1][c, :, 0])) for c in opened}, audio[1]))
    return out


def check(results):
    """What the example promises: on every open channel the hum is down by the filter's attenuation at the tone, give or
    take 3 dB, and the closed rows are exact zeros still."""
    want = attenuation_db(VOICE_NFM)
    for opened, hum, audio in results:
        assert len(opened) == 2, opened
        for c in range(audio.shape[0]):
            if c in opened:
                before, after = hum[c]
                assert before - after >= want - 3.0, (c, before, after, want)
                assert np.abs(audio[c]).max() > 1e-4, c
            else:
                assert not audio[c].any(), c


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--rate", type=int, default=1_000_000)
    ap.add_argument("--seconds", type=int, default=2)
    a = ap.parse_args()
    t0 = time.perf_counter()
    results = run(a.channels, a.rate, a.seconds)
    check(results)
    print("the voice filter takes %.1f dB off %.1f Hz" % (attenuation_db(VOICE_NFM), pmr.WANTED))
    for k, (opened, hum, _) in enumerate(results):
        print("second %d: %s" % (k, "; ".join("channel %d hum %.1f dB -> %.1f dB" % (c, *hum[c]) for c in opened)))
    print("%.2f s wall" % (time.perf_counter() - t0))
