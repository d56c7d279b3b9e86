#!/usr/bin/env python3
"""The airband receiver of examples/airband_am.py fed the way a receiver delivers samples: interleaved int16.

The synthetic airband buffer is quantised to int16 (cs16: Airspy, the USRP wire format, most recordings) in page-locked
memory.  One loop hands it to the GPU as it is -- `Feeder(2 N, "int16")` -> `Tuner.load_raw` -> `run_all` -- and the
conversion to float rides on the first pass of the wideband FFT: 4 bytes per sample cross PCIe and are read once.  Next
to it runs what a host had to do before: widen the buffer to complex64 in numpy (8 bytes per sample), feed that, `load`.
Both conversions are exact (an int16 times 2^-15 is a float32), so the audio of the two loops is identical, bit for bit.

    python examples/airband_cs16.py [--channels 760] [--rate 20000000] [--seconds 2]
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
from radiocore.tools import Buffer, Feeder  # noqa: E402

_spec = importlib.util.spec_from_file_location("airband_am", os.path.join(ROOT, "examples", "airband_am.py"))
airband_am = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(airband_am)
CHANNEL, AUDIO = airband_am.CHANNEL, airband_am.AUDIO


def quantise(x, out):
    """complex64 [N] -> interleaved int16 [2 N] in `out`, the strongest component at 90 % of full scale (what an ADC's
    gain control aims for)."""
    iq = x.view(np.float32)
    np.rint(iq * (0.9 * 32767.0 / float(np.max(np.abs(iq)))), out=iq)
    out[:] = iq.astype(np.int16)


def run(channels=760, rate=20_000_000, seconds=2):
    """Returns (identical, audio, host_ms): whether every second's audio of the raw loop equals the complex64 loop's bit
    for bit, the raw loop's audio, [seconds][C, A, 1] float32, and what the host's own conversion of each buffer took."""
    n = int(rate)
    first = 118_012_500.0
    centres = [first + CHANNEL * i for i in range(channels)]
    tuners = []
    for _ in range(2):                             # one receiver per loop: same channels, own device handles
        t = Tuner(cuda=True)
        for f in centres:
            t.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
        t.request_bandwidth(float(rate))
        tuners.append(t)
    raw_tuner, wide_tuner = tuners
    rng = np.random.default_rng(118)
    raw = [Buffer(2 * n, "int16", cuda=True) for _ in range(seconds)]          # page-locked, as a receiver's driver fills it
    wide = [Buffer(n, "complex64", cuda=True) for _ in range(seconds)]
    host_ms = []
    for second in range(seconds):
        x, _, _ = airband_am.airband(rate, centres, raw_tuner.input_frequency, second, rng)
        quantise(x, raw[second].data)
        t0 = time.perf_counter()                   # the host conversion load_raw makes unnecessary
        wide[second].data.view(np.float32)[:] = raw[second].data.astype(np.float32) * np.float32(2.0 ** -15)
        host_ms.append(1e3 * (time.perf_counter() - t0))

    def loop(feeder, buffers, tuner, load):
        audio = []
        feeder.submit(buffers[0].data)
        for i in range(seconds):
            if i + 1 < seconds:
                feeder.submit(buffers[i + 1].data)
            with feeder.next() as dev:
                load(dev)
                audio.append(tuner.run_all())
        feeder.close()
        return audio

    got = loop(Feeder(2 * n, "int16"), raw, raw_tuner, raw_tuner.load_raw)
    want = loop(Feeder(n, "complex64"), wide, wide_tuner, wide_tuner.load)
    identical = all(np.array_equal(g, w) for g, w in zip(got, want))
    return identical, got, host_ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--seconds", type=int, default=2)
    a = ap.parse_args()
    identical, audio, host_ms = run(a.channels, a.rate, a.seconds)
    print("%d s x %d channels from int16 (%.0f MB per buffer instead of %.0f MB): audio of load_raw and of load "
          "(host conversion %.0f ms per buffer) is %s" %
          (a.seconds, a.channels, 4e-6 * a.rate, 8e-6 * a.rate, float(np.median(host_ms)),
           "identical" if identical else "DIFFERENT"))
    sys.exit(0 if identical else 1)
