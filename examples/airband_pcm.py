#!/usr/bin/env python3
"""The publisher's side of a squelched band monitor: int16 PCM of the open channels only, drained under compute.  No SDR
or sound card.

The band is the one of examples/airband_squelch.py: VHF airband, 760 channels of 25 kHz, a dozen AM stations on the air.
There `run_all()` brings all 760 rows of float32 audio to the host and `wire.frames(open_mask=...)` throws the closed ones
away.  Here `Tuner.run_all_packed(PCM("int16"), drain=...)` converts and compacts on the device, a `Drain` of depth 2
copies the header and the open rows to page-locked memory while the next buffer's kernels run, and
`wire.frames_packed` turns the rows into the messages a sound device or codec wants.  Every payload is checked against the
numpy quantisation of `run_all()`'s float32 audio of the same buffer.

    python examples/airband_pcm.py [--small] [--channels 760] [--rate 20000000] [--buffers 3] [--stations 12]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "radio-core_amd"), HERE]

import numpy as np  # noqa: E402

from airband_squelch import AUDIO, CHANNEL, OVER_FLOOR_DB, band  # noqa: E402
from radiocore import AM, PCM, Tuner  # noqa: E402
from radiocore.tools import Drain, squelch, wire  # noqa: E402

SMALL = dict(channels=120, rate=4_000_000, stations=7)      # a geometry that runs in a few seconds


def quantise(audio, gain):
    """What PCM("int16", gain) asks of the device, in numpy: one float32 multiply, NaN -> 0, round to nearest even,
    clamp to +-32767."""
    y = np.asarray(audio, np.float32) * np.float32(gain)
    return np.where(np.isnan(y), np.float32(0), np.clip(np.rint(y), -32767, 32767)).astype(np.int16)


def run(channels=760, rate=20_000_000, buffers=3, stations=12, publish=None):
    """Returns (opened, planted, messages): per buffer the channel indices that produced a message and the ones that were
    on the air, and every published (frequency, int16 [A, 1])."""
    first = 118_012_500.0                          # the centre of the first 25 kHz airband channel
    centres = [first + CHANNEL * i for i in range(channels)]
    tuner = Tuner(cuda=True)
    for f in centres:
        tuner.add_channel(f, CHANNEL, AM(CHANNEL, AUDIO, cuda=True))
    tuner.request_bandwidth(float(rate))
    rng = np.random.default_rng(121)
    pcm = PCM("int16", 32767.0)
    drain = Drain(channels, (AUDIO, 1), "int16", depth=2)
    opened, planted, out, expected = [], [], [], []

    def publish_oldest():
        # the oldest buffer in flight: waits for its header, copies its open rows, frames them
        with drain.next() as (index, audio):
            want_index, want_rows = expected.pop(0)
            assert np.array_equal(index, want_index), "closed channels produce no message, open ones all do"
            messages = wire.frames_packed(tuner.channels(), index, audio)
            for k, message in enumerate(messages):
                assert message[1] == want_rows[k].tobytes(), "payload differs from the quantised float32 audio"
                if publish is not None:
                    publish(message)               # socket.send_multipart(message) in a server
                out.append(wire.parse_frame(message, 1, dtype=np.int16))
            opened.append([int(c) for c in index])

    for i in range(buffers):
        on_air = sorted(int(c) for c in rng.choice(channels, stations, replace=False))
        tuner.load(band(rate, centres, tuner.input_frequency, on_air, rng))
        if i == 0:
            # calibration: the median power density over the channels is the floor, whoever is on the air meanwhile
            tuner.set_squelch(squelch.threshold_over_floor(tuner.levels(), CHANNEL, OVER_FLOOR_DB))
        tuner.run_all_packed(pcm, drain=drain)     # kernels, pack and header copy of buffer i: queued, not waited for
        # the check's reference (a publisher would not run this): AM keeps no state, the same buffer runs again
        ref = tuner.run_all(numpy_output=True)
        mask = tuner.open_mask()
        expected.append((np.flatnonzero(mask).astype(np.int32), quantise(ref[mask], pcm.gain)))
        planted.append(on_air)
        if i > 0:
            publish_oldest()                       # buffer i - 1, while buffer i is in flight
    publish_oldest()
    drain.close()
    return opened, planted, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--channels", type=int, default=760)
    ap.add_argument("--rate", type=int, default=20_000_000)
    ap.add_argument("--buffers", type=int, default=3)
    ap.add_argument("--stations", type=int, default=12)
    a = ap.parse_args()
    geo = SMALL if a.small else dict(channels=a.channels, rate=a.rate, stations=a.stations)
    t0 = time.perf_counter()
    opened, planted, msgs = run(buffers=a.buffers, **geo)
    for k, (o, p) in enumerate(zip(opened, planted)):
        print("buffer %d: open %s  (on the air: %s)%s" % (k, o, p, "" if o == p else "  MISMATCH"))
    rows = sum(len(o) for o in opened)
    print("%d int16 frames published (%d bytes) instead of %d float32 rows (%d bytes), %.2f s wall"
          % (len(msgs), rows * AUDIO * 2, geo["channels"] * len(opened), geo["channels"] * len(opened) * AUDIO * 4,
             time.perf_counter() - t0))
