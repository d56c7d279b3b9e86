#!/usr/bin/env python3
"""A multi-channel AM receiver: VHF airband (118-137 MHz, 25 kHz channels) out of one wideband buffer, no SDR or
sound card.

A synthetic one-second buffer holds an AM station on every channel, at levels 20 dB apart and with their carriers up
to 1 kHz off the channel centre.  One `Tuner` carries an `AM` demodulator per channel; `run_all()` demodulates every
channel in one batched call, and `radiocore.tools.wire` cuts the result into the per-channel messages of the
multi-channel server (examples/multi_fm_pipeline.py).  AM normalises every channel by its own carrier level, so a
tone at modulation index m comes out at amplitude m whatever the station's level.

    python examples/airband_am.py [--channels 760] [--rate 20000000] [--seconds 2]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AM, Tuner  # noqa: E402
from radiocore.tools import wire  # noqa: E402

CHANNEL = 25_000       # channel raster and bandwidth (Hz)
AUDIO = 8_000          # audio rate (Hz)


def airband(rate, centres, f_in, second, rng):
    """One second of complex baseband at `rate` samples/s: station i is an AM carrier at centres[i], modulated by a
    voice-band tone at index m_i, at its own level and carrier offset.  Returns (iq complex64, m, tone)."""
    n = int(rate)
    X = np.zeros(n, np.complex128)
    t = np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    m = rng.uniform(0.3, 0.8, len(centres))
    tone = 300.0 + (37.0 * np.arange(len(centres))) % 3000.0 + 50.0 * second      # 300 .. 3350 Hz
    level = 10.0 ** rng.uniform(-1.0, 0.0, len(centres))
    offset = rng.integers(-1000, 1001, len(centres))
    for i, fc in enumerate(centres):
        s = level[i] * (1 + m[i] * np.sin(2 * np.pi * tone[i] * t)) * np.exp(2j * np.pi * offset[i] * t)
        X[(kk + int(fc - f_in)) % n] += np.fft.fft(s) * (n / CHANNEL)      # the station's bins in the wide band
    x = np.fft.ifft(X)
    x += 1e-4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64), m, tone


def run(channels=760, rate=20_000_000, seconds=2, publish=None):
    """Returns [(frequency, float32 [A, 1])] per second and channel, in publish order, and the worst deviation of
    a channel's tone amplitude from its modulation index."""
    first = 118_012_500.0                          # the centre of the first 25 kHz airband channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))           # 19 MHz of channels, an FFT-friendly 20 MSPS buffer
    rng = np.random.default_rng(118)
    out, worst = [], 0.0
    k = np.arange(AUDIO)
    for second in range(seconds):
        x, m, tone = airband(rate, centres, tuner.input_frequency, second, rng)
        tuner.load(x)
        audio = tuner.run_all()                    # [C, A, 1] float32: every channel's envelope, one call
        for message in wire.frames(tuner.channels(), audio):
            if publish is not None:
                publish(message)                   # socket.send_multipart(message) in a server
            out.append(wire.parse_frame(message, 1))
        # each channel's tone, measured by projection, sits at its modulation index (up to the decimator's window)
        for i in range(0, channels, max(1, channels // 16)):
            ref = np.exp(-2j * np.pi * tone[i] * k / AUDIO)
            amp = 2 * abs(np.dot(audio[i, :, 0], ref)) / AUDIO
            w = 0.54 + 0.46 * np.cos(2 * np.pi * tone[i] / CHANNEL)
            worst = max(worst, abs(amp - m[i] * w))
    return out, worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=int, default=2)
    a = ap.parse_args()
    t0 = time.perf_counter()
    msgs, worst = run(a.channels, a.rate, a.seconds)
    dt = time.perf_counter() - t0
    print("%d messages (%d s x %d channels), %.1f MB of audio, tone amplitude within %.1e of m, %.2f s wall" %
          (len(msgs), a.seconds, a.channels, sum(p.nbytes for _, p in msgs) / 1e6, worst, dt))
