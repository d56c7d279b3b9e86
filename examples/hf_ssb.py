#!/usr/bin/env python3
"""A multi-channel SSB receiver: an HF voice band out of one wideband buffer, no SDR or sound card.

A synthetic one-second buffer at 2 MSPS holds a single-sideband station on every 12.5 kHz channel around 10 MHz.  By the
amateur convention the stations below 10 MHz transmit the lower sideband and those above it the upper one, and every
other station is 12 dB weaker than its neighbours.  One `Tuner` carries an `LSB` or `USB` demodulator per channel:
`run_each()` demodulates each sideband's block of channels in one batched call straight from the loaded spectrum
(`--plan usb` / `--plan lsb`: one class everywhere and `run_all()`), and `radiocore.tools.wire` cuts the result into the
per-channel messages of the multi-channel server (examples/multi_fm_pipeline.py).  SSB normalises every channel to an
audio RMS of 0.25, so a station's single tone comes out at amplitude 0.354 whatever its level -- and the opposite
sideband of the same channel holds nothing but the noise floor.

    python examples/hf_ssb.py [--channels 150] [--rate 2000000] [--seconds 2] [--plan split|usb|lsb]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import LSB, USB, Tuner  # noqa: E402
from radiocore.tools import wire  # noqa: E402

CHANNEL = 12_500       # channel raster and bandwidth (Hz)
AUDIO = 8_000          # audio rate (Hz)
LEVEL = 0.25           # RCFM_SSB_LEVEL: the audio RMS of every channel


def hf_band(rate, centres, lower, f_in, second, rng):
    """One second of complex baseband at `rate` samples/s: station i is one voice-band tone in the sideband lower[i]
    says, `tone[i]` Hz from its suppressed carrier centres[i], over its own noise floor.  Returns (iq complex64, tone)."""
    n = int(rate)
    X = np.zeros(n, np.complex128)
    t = np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    tone = 300.0 + (37.0 * np.arange(len(centres))) % 2400.0 + 50.0 * second      # 300 .. 2750 Hz
    for i, fc in enumerate(centres):
        level = 1.0 if i % 2 == 0 else 0.25
        s = np.exp((-2j if lower[i] else 2j) * np.pi * tone[i] * t)
        s = level * (s + 0.01 * (rng.standard_normal(CHANNEL) + 1j * rng.standard_normal(CHANNEL)))
        X[(kk + int(fc - f_in)) % n] += np.fft.fft(s) * (n / CHANNEL)      # the station's bins in the wide band
    x = np.fft.ifft(X)
    x += 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), tone


def run(channels=150, rate=2_000_000, seconds=2, plan="split", publish=None):
    """Returns [(frequency, float32 [A, 1])] per second and channel, in publish order, and the worst deviation of a
    channel's tone amplitude from LEVEL sqrt(2)."""
    centres = [10_000_000.0 + CHANNEL * (i - channels // 2) + CHANNEL // 2 for i in range(channels)]
    lower = [f < 10e6 if plan == "split" else plan == "lsb" for f in centres]
    tuner = Tuner(cuda=True)
    for f, lo in zip(centres, lower):
        tuner.add_channel(f, CHANNEL, (LSB if lo else USB)(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    rng = np.random.default_rng(40)
    out, worst = [], 0.0
    k = np.arange(AUDIO)
    for second in range(seconds):
        x, tone = hf_band(rate, centres, lower, tuner.input_frequency, second, rng)
        tuner.load(x)
        if plan == "split":
            audio = np.stack(tuner.run_each())     # one batched call per sideband block
        else:
            audio = tuner.run_all()                # [C, A, 1] float32, one call
        for message in wire.frames(tuner.channels(), audio):
            if publish is not None:
                publish(message)                   # socket.send_multipart(message) in a server
            out.append(wire.parse_frame(message, 1))
        # each channel's tone, measured by projection, sits at LEVEL sqrt(2) (less what the noise takes of the RMS)
        for i in range(0, channels, max(1, channels // 16)):
            ref = np.exp(-2j * np.pi * tone[i] * k / AUDIO)
            amp = 2 * abs(np.dot(audio[i, :, 0], ref)) / AUDIO
            worst = max(worst, abs(amp - LEVEL * np.sqrt(2.0)))
    return out, worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=150)
    ap.add_argument("--rate", type=int, default=2_000_000)
    ap.add_argument("--seconds", type=int, default=2)
    ap.add_argument("--plan", choices=("split", "usb", "lsb"), default="split")
    a = ap.parse_args()
    t0 = time.perf_counter()
    msgs, worst = run(a.channels, a.rate, a.seconds, a.plan)
    dt = time.perf_counter() - t0
    print("%d messages (%d s x %d channels), %.1f MB of audio, tone amplitude within %.1e of %.3f, %.2f s wall" %
          (len(msgs), a.seconds, a.channels, sum(p.nbytes for _, p in msgs) / 1e6, worst, LEVEL * np.sqrt(2.0), dt))
