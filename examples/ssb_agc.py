#!/usr/bin/env python3
"""An SSB band monitor that can be listened to: the AGC carried from buffer to buffer, next to the per-buffer RMS.

Three one-second buffers at 2 MSPS hold an upper-sideband station on every 12.5 kHz channel of an HF band, each sending
one voice-band tone at its own level (every other station 12 dB weaker).  The stations on odd channels pause for the
second half of buffer 1.  Two Tuners demodulate the same buffers, one with `USB(..., agc=AGC(decay=1.0))` and one
without.  Without, every buffer is normalised by its own RMS: the half-silent buffer comes out 3 dB louder than its
neighbours, and the gain steps at both of its ends.  With, the peak follower holds the station's level through the pause
and every buffer plays the tone at `level`, whatever the station's strength.

    python examples/ssb_agc.py [--channels 40] [--rate 2000000]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AGC, USB, Tuner  # noqa: E402

CHANNEL = 12_500       # channel raster and bandwidth (Hz)
AUDIO = 8_000          # audio rate (Hz)
LEVEL = 0.25           # what the AGC scales a station's peak to


def hf_band(rate, centres, f_in, second, rng):
    """One second of complex baseband at `rate` samples/s: station i sends tone[i] Hz above its suppressed carrier;
    in second 1 the stations on odd channels fall silent after 0.48 s (a 20 ms raised-cosine fall)."""
    n = int(rate)
    X = np.zeros(n, np.complex128)
    t = np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    tone = 400.0 + (37.0 * np.arange(len(centres))) % 2200.0
    gate = 0.5 - 0.5 * np.cos(np.pi * np.clip((0.5 - t) / 0.02, 0.0, 1.0))
    for i, fc in enumerate(centres):
        level = 1.0 if i % 4 < 2 else 0.25
        s = np.exp(2j * np.pi * tone[i] * t) * (gate if (second == 1 and i % 2) else 1.0)
        s = level * (s + 1e-3 * (rng.standard_normal(CHANNEL) + 1j * rng.standard_normal(CHANNEL)))
        X[(kk + int(fc - f_in)) % n] += np.fft.fft(s) * (n / CHANNEL)
    x = np.fft.ifft(X)
    x += 1e-5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), tone


def run(channels=40, rate=2_000_000):
    """Returns the tone amplitude per (tuner, buffer, channel) over the first 0.4 s of each buffer: [2, 3, channels]."""
    centres = [10_000_000.0 + CHANNEL * (i - channels // 2) + CHANNEL // 2 for i in range(channels)]
    tuners = []
    for agc in (AGC(decay=1.0, level=LEVEL, floor=1e-3), None):
        t = Tuner(cuda=True)
        for f in centres:
            t.add_channel(f, CHANNEL, USB(CHANNEL, AUDIO, cuda=True, agc=agc))
        t.request_bandwidth(float(rate))
        tuners.append(t)
    rng = np.random.default_rng(41)
    k = np.arange(int(0.05 * AUDIO), int(0.40 * AUDIO))
    amp = np.zeros((2, 3, channels))
    for second in range(3):
        x, tone = hf_band(rate, centres, tuners[0].input_frequency, second, rng)
        for j, t in enumerate(tuners):
            t.load(x)
            audio = t.run_all()                         # [C, A, 1] float32
            probe = np.exp(-2j * np.pi * np.outer(tone, k) / AUDIO)
            amp[j, second] = 2.0 * np.abs(np.mean(audio[:, k, 0] * probe, axis=1))
    return amp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=40)
    ap.add_argument("--rate", type=int, default=2_000_000)
    a = ap.parse_args()
    amp = run(a.channels, a.rate)
    paused = np.arange(a.channels) % 2 == 1
    for j, name in enumerate(("with agc", "per-buffer RMS")):
        for label, sel in (("steady stations", ~paused), ("pausing stations", paused)):
            db = 20 * np.log10(amp[j][:, sel] / amp[j][0, sel])
            print("%-15s %-17s tone amplitude per buffer %s   buffer 1 against buffer 0: %+.2f dB"
                  % (name, label, np.round(amp[j][:, sel].mean(axis=1), 4).tolist(), db[1].mean()))
    agc_dev = np.max(np.abs(amp[0] / LEVEL - 1.0))
    rms_step = np.min(np.abs(20 * np.log10(amp[1][1, paused] / amp[1][0, paused])))
    print("with agc: every tone within %.2f %% of level %.2f; per-buffer RMS: the pause moves its buffer by %.2f dB"
          % (100 * agc_dev, LEVEL, rms_step))
    if not (agc_dev <= 0.01 and rms_step > 2.0):
        raise SystemExit("the AGC did not hold the level")


if __name__ == "__main__":
    main()
