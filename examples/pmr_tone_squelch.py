#!/usr/bin/env python3
"""A tone squelch: narrow-FM channels shared by several user groups that tell each other apart by CTCSS tone, no SDR or
sound card.

A level squelch answers "is there power in this channel"; on a shared PMR or repeater channel the question is "is this
transmission for me".  Every transmitter adds a sub-audible tone (67 .. 254 Hz) to its speech, and a receiver opens only
for its own group's tone.  Here one `ToneBank` of the 39 CTCSS tones runs on the device behind the FM demodulators of every
channel, `set_tones(bank, want=..., ratio=...)` turns it into a squelch, `open_mask()` tells which channels to publish,
and `tones.strongest` names the tone each station carries.

    python examples/pmr_tone_squelch.py [--channels 16] [--rate 1000000] [--seconds 2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import FM, ToneBank, Tuner  # noqa: E402
from radiocore.tools import tones  # noqa: E402

CHANNEL = 12_500       # channel raster and bandwidth (Hz)
AUDIO = 8_000          # audio rate (Hz)
DEVIATION = 2_500.0    # peak frequency deviation (Hz) of a full-scale message
WANTED = 88.5          # our group's tone (Hz)
RATIO = 0.01           # open when the wanted tone holds at least this share of the audio power


def speech(rng):
    """Noise-like speech at the channel rate: Gaussian, 300 .. 3000 Hz, standard deviation 0.2."""
    S = np.fft.rfft(rng.standard_normal(CHANNEL))
    f = np.fft.rfftfreq(CHANNEL, 1.0 / CHANNEL)
    S[(f < 300.0) | (f > 3000.0)] = 0.0
    s = np.fft.irfft(S, CHANNEL)
    return 0.2 * s / np.std(s)


def band(rate, centres, f_in, on_air, rng):
    """One second of complex baseband at `rate` samples/s: on each channel of `on_air` ({channel: tone in Hz}) an FM
    station, speech plus its CTCSS tone at amplitude 0.1, at levels up to 20 dB apart; receiver noise everywhere."""
    n = int(rate)
    X = np.zeros(n, np.complex128)
    t = np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    for i, tone in on_air.items():
        m = speech(rng) + 0.1 * np.cos(2 * np.pi * tone * t + rng.uniform(0, 2 * np.pi))
        s = 10.0 ** rng.uniform(-1.0, 0.0) * np.exp(2j * np.pi * DEVIATION * np.cumsum(m) / CHANNEL)
        X[(kk + int(centres[i] - f_in)) % n] += np.fft.fft(s) * (n / CHANNEL)
    x = np.fft.ifft(X)
    x += 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def run(channels=16, rate=1_000_000, seconds=2):
    """Returns one (on_air, opened, named, audio) per second: {channel: tone in Hz} of the stations on the air, the
    channels the tone squelch opened, {channel: tone in Hz} as `tones.strongest` names them, and the audio [C, A, 1]."""
    first = 446_006_250.0                          # the centre of the first 12.5 kHz PMR446 channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, FM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    bank = ToneBank(tones.CTCSS)                   # one frame per buffer, Hann window
    tuner.set_tones(bank, want=WANTED, ratio=RATIO)
    rng = np.random.default_rng(446)
    out = []
    for second in range(seconds):
        # five stations per second, two of them of our group; the other channels are empty
        where = sorted(int(i) for i in rng.choice(channels, 5, replace=False))
        other = rng.choice([f for f in tones.CTCSS if f != WANTED], 3, replace=False)
        on_air = dict(zip(where, [WANTED, float(other[0]), float(other[1]), WANTED, float(other[2])]))
        tuner.load(band(rate, centres, tuner.input_frequency, on_air, rng))
        audio = tuner.run_all()                    # [C, A, 1]: everything but our group's channels is exact zeros
        mask = tuner.open_mask()
        P, E = tuner.tone_power()
        best = tones.strongest(P, E, RATIO)[:, 0, 0]
        named = {int(c): tones.CTCSS[int(k)] for c, k in enumerate(best) if k >= 0}
        out.append((on_air, [int(i) for i in np.flatnonzero(mask)], named, audio))
    return out


def check(results):
    """What the example promises: only the channels that carry the wanted tone are open, closed rows are exact zeros,
    and `strongest` names each station's tone (and none on an empty channel)."""
    for on_air, opened, named, audio in results:
        assert opened == sorted(c for c, f in on_air.items() if f == WANTED), (opened, on_air)
        for c in range(audio.shape[0]):
            if c in opened:
                assert np.abs(audio[c]).max() > 1e-3, c
            else:
                assert not audio[c].any(), c
        assert named == on_air, (named, on_air)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--rate", type=int, default=1_000_000)
    ap.add_argument("--seconds", type=int, default=2)
    a = ap.parse_args()
    t0 = time.perf_counter()
    results = run(a.channels, a.rate, a.seconds)
    check(results)
    for k, (on_air, opened, named, _) in enumerate(results):
        print("second %d: open %s for %.1f Hz; on the air: %s" % (k, opened, WANTED, ", ".join("%d: %.1f Hz" % cf for cf in sorted(named.items()))))
    print("%.2f s wall" % (time.perf_counter() - t0))
