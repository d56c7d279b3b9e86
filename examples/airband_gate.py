#!/usr/bin/env python3
"""A band monitor whose squelch is right to 20 ms: VHF airband (760 channels of 25 kHz), stations that key on and off in the
middle of the one-second buffers, no SDR or sound card.

`Tuner.set_squelch` decides once per buffer: a transmission that starts 0.3 s into a buffer either opens the whole second
(0.3 s of noise goes out with it, and the rest of the second after it ends) or -- when its share of the second is too small
to lift the channel's mean level over the threshold -- is lost.  `Tuner.set_gate` with a `FrameGate` cuts every buffer
into 50 frames, opens with the frame before the first one over the threshold, holds through a speaker's pause, and keeps
its state from buffer to buffer; `frame_mask()` and `squelch.segments` give the publisher the runs of samples to send.
Both rules run here over the same three buffers, and the example counts what each published, lost and let through.

    python examples/airband_gate.py [--channels 760] [--rate 20000000] [--stations 12]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd")]

import numpy as np  # noqa: E402

from radiocore import AM, FrameGate, Tuner  # noqa: E402
from radiocore.tools import squelch  # noqa: E402

CHANNEL = 25_000       # channel raster and bandwidth (Hz)
AUDIO = 8_000          # audio rate (Hz)
SECONDS = 3
FRAMES = 50            # 20 ms
OVER_FLOOR_DB = 10.0


def transmissions(channels, stations, rng):
    """{channel: [(start s, stop s)]}: one or two transmissions per station somewhere in the three seconds, the second one a
    pause of 0.1 s behind the first (shorter than the gate's hang time)."""
    out = {}
    for i in sorted(int(i) for i in rng.choice(channels, stations, replace=False)):
        start = float(rng.uniform(0.05, SECONDS - 0.6))
        length = float(rng.uniform(0.15, 1.2))
        stop = min(start + length, SECONDS - 0.35)
        runs = [(start, stop)]
        if rng.random() < 0.5 and stop + 0.3 < SECONDS - 0.35:
            runs.append((stop + 0.1, stop + 0.3))
        out[i] = runs
    return out


def band(rate, centres, f_in, on_air, second, rng):
    """Second `second` of complex baseband at `rate` samples/s: every station of `on_air` an AM carrier with one voice-band
    tone, keyed by its transmissions, and receiver noise everywhere."""
    n = int(rate)
    X = np.zeros(n, np.complex128)
    t = second + np.arange(CHANNEL) / CHANNEL
    kk = np.fft.fftfreq(CHANNEL, 1.0 / CHANNEL).astype(np.int64)
    for i, runs in on_air.items():
        key = np.zeros(CHANNEL)
        for a, b in runs:
            key[(t >= a) & (t < b)] = 1.0
        if not key.any():
            continue
        tone = 300.0 + (37.0 * i) % 3000.0
        s = 0.3 * key * (1 + 0.5 * np.sin(2 * np.pi * tone * t)) * np.exp(2j * np.pi * (i % 7 - 3) * 100 * t)
        X[(kk + int(centres[i] - f_in)) % n] += np.fft.fft(s) * (n / CHANNEL)
    x = np.fft.ifft(X)
    x += 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def account(sent, wanted):
    """(published, lost, let through) in audio samples: `sent` and `wanted` are bool [C, SECONDS AUDIO]."""
    return int(sent.sum()), int((wanted & ~sent).sum()), int((sent & ~wanted).sum())


def run(channels=760, rate=20_000_000, stations=12, publish=None):
    """Both rules over the same three buffers.  Returns {"squelch": (published, lost, let through), "gate": (...)} in audio
    samples, the gate's segments [(second, channel, start, stop)] and the transmissions {channel: [(start s, stop s)]}."""
    first = 118_012_500.0                          # the centre of the first 25 kHz airband channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuners = []
    for _ in range(2):
        tuner = Tuner(cuda=True)
        for f in centres:
            tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
        tuner.request_bandwidth(float(rate))
        tuners.append(tuner)
    by_buffer, by_frame = tuners
    rng = np.random.default_rng(122)
    on_air = transmissions(channels, stations, rng)
    gate = FrameGate(frames=FRAMES, hang=0.25, lead=1, ramp=0.005)
    sent_buffer = np.zeros((channels, SECONDS * AUDIO), bool)
    sent_frame = np.zeros_like(sent_buffer)
    published = []
    for second in range(SECONDS):
        x = band(rate, centres, by_buffer.input_frequency, on_air, second, rng)
        by_buffer.load(x)
        by_frame.load(x)
        if second == 0:
            # calibration: the median power density over the channels is the floor, whoever is on the air meanwhile
            thresholds = squelch.threshold_over_floor(by_buffer.levels(), CHANNEL, OVER_FLOOR_DB)
            by_buffer.set_squelch(thresholds)
            by_frame.set_gate(gate, open=thresholds)           # close: 3 dB below
        by_buffer.run_all()
        sent_buffer[by_buffer.open_mask(), second * AUDIO:(second + 1) * AUDIO] = True
        audio = by_frame.run_all()                              # [C, A, 1]: closed frames are exact zeros
        for c, start, stop in squelch.segments(by_frame.frame_mask(), AUDIO):
            sent_frame[c, second * AUDIO + start:second * AUDIO + stop] = True
            published.append((second, c, start, stop))
            if publish is not None:
                publish([by_frame.channels()[c].address_bytes, audio[c, start:stop].tobytes()])
    wanted = np.zeros_like(sent_buffer)
    for c, runs in on_air.items():
        for a, b in runs:
            wanted[c, int(np.floor(a * AUDIO)):int(np.ceil(b * AUDIO))] = True
    return {"squelch": account(sent_buffer, wanted), "gate": account(sent_frame, wanted)}, published, on_air


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--stations", type=int, default=12)
    a = ap.parse_args()
    t0 = time.perf_counter()
    totals, published, on_air = run(a.channels, a.rate, a.stations)
    on = sum(b - c for runs in on_air.values() for c, b in runs)
    print("%d stations, %.2f s of speech in all, %d segments published by the gate" % (len(on_air), on, len(published)))
    for rule, (sent, lost, extra) in totals.items():
        print("%-8s published %6.2f s   lost %5.2f s   let through %5.2f s of an empty channel"
              % (rule, sent / AUDIO, lost / AUDIO, extra / AUDIO))
    print("%.2f s wall" % (time.perf_counter() - t0))
