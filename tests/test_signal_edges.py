"""No GPU: pins the inputs of tests/test_hip_signal_edges.py, so that the GPU tests cannot pass or fail on an
ill-conditioned signal.  Every band of signal_edges.GEOMETRIES, as the oracle's Tuner hands it to the demodulators
(run_pruned), over the consecutive buffers the GPU tests run:

    step bound      max |phase step| <= 0.85 pi: the discriminator is nowhere near its wrap
    clip stations   1 % .. 10 % of the truth's samples sit at the intended bound, none at the other one
    DC stations     the pre-removal mean is within 10 % of `level`, and no sample is within 0.05 of +-0.999 -- outside
                    the first 50 samples of the first buffer: a fresh de-emphasis filter starts from lfilter_zi
                    (deemphasis.py:48), the state a unit step leaves, so the reference's own first samples of a
                    channel are ~1 - mean whatever the signal (1.4 at level -0.4: clipped, far from the bound)
    conditioning    moving every input sample by 1e-7 of its magnitude moves the truth by at most 1e-6 of its peak
    boundary cap    at most 0.1 % of the truth's unclipped samples lie within 1e-5 of +-0.999 (only those may be
                    clipped on one side of a comparison and not on the other)

and the truth itself: signal_edges.Truth is the oracle with its discriminator patched, bit for bit.
"""

import numpy as np
import pytest

import radiocore_oracle as oracle
import signal_edges as se

IDS = ["%s-%d-%d" % (g[0], g[2], g[3]) for g in se.GEOMETRIES]


@pytest.mark.parametrize("geometry", se.GEOMETRIES, ids=IDS)
def test_clipping_bands(geometry):
    kind, N, B, A, C = geometry
    bufs = se.evaluate("clip", geometry, perturb=1e-7)
    assert len(bufs) >= 3
    seen = set()
    for b, rec in enumerate(bufs):
        seen.update(rec["tags"])
        for i, sign in enumerate(rec["tags"]):
            step = float(np.max(np.abs(se.steps(rec["iq"][i]))))
            un = rec["unclipped"][i]
            hi, lo = float(np.mean(un >= se.CLIP)), float(np.mean(un <= -se.CLIP))
            near = float(np.mean(np.abs(np.abs(un) - se.CLIP) <= 1e-5))
            print(kind, B, A, "buf", b, "ch", i, "sign", sign, "step %.3f hi %.4f lo %.4f near %.5f cond %.2e"
                  % (step, hi, lo, near, rec["cond"][i]))
            assert step <= se.STEP_BOUND, (b, i, step)
            assert rec["cond"][i] <= 1e-6, (b, i, rec["cond"][i])
            assert near <= 1e-3, (b, i, near)
            if sign:
                mine, other = (hi, lo) if sign > 0 else (lo, hi)
                assert 0.01 <= mine <= 0.10, (b, i, sign, mine)
                assert other == 0.0, (b, i, sign, other)
                t = rec["truth"][i]
                assert (np.max(t) == se.CLIP) if sign > 0 else (np.min(t) == -se.CLIP)
    assert seen == {1, -1, 0}, seen            # both bounds and an ordinary station in one band


@pytest.mark.parametrize("geometry", se.GEOMETRIES, ids=IDS)
def test_dc_bands(geometry):
    kind, N, B, A, C = geometry
    bufs = se.evaluate("dc", geometry, perturb=1e-7)
    assert len(bufs) >= 3
    seen = set()
    for b, rec in enumerate(bufs):
        seen.update(rec["tags"])
        for i, level in enumerate(rec["tags"]):
            step = float(np.max(np.abs(se.steps(rec["iq"][i]))))
            un = rec["unclipped"][i][50 if b == 0 else 0:]
            peak = float(np.max(np.abs(un)))
            print(kind, B, A, "buf", b, "ch", i, "level", level, "step %.3f mean %.4f peak %.3f cond %.2e"
                  % (step, rec["mean"][i], peak, rec["cond"][i]))
            assert step <= se.STEP_BOUND, (b, i, step)
            assert rec["cond"][i] <= 1e-6, (b, i, rec["cond"][i])
            assert abs(rec["mean"][i] - level) <= 0.1 * abs(level), (b, i, rec["mean"][i])
            assert peak <= se.CLIP - 0.05, (b, i, peak)
            # the last 50 audio samples carry signal: the tail term of the derived mean is not multiplied by zeros
            tail = rec["unclipped"][i][-50:]
            assert float(np.max(tail) - np.min(tail)) >= 0.05, (b, i)
    assert seen == set(se.DC_LEVELS), seen


@pytest.mark.parametrize("kind", ["FM", "MFM", "WBFM"])
def test_truth_is_the_oracle_with_the_float64_discriminator(kind, monkeypatch):
    """What test_off_raster_stations_through_run_all patches into the oracle, buffer after buffer (carried state)."""
    B, A = 60000, 12000
    monkeypatch.setattr(oracle, "discriminator", se.steps)
    patched, mine = getattr(oracle, kind)(B, A), se.truth(kind, B, A)
    for buf in range(2):
        iq = se.clipping_station(B, 5 + buf, 1 - 2 * buf, stereo=(kind == "WBFM"))
        want = np.asarray(patched.run(iq)).reshape(A, mine.ch)
        assert np.array_equal(mine.run(iq), want), (kind, buf)


def test_generators_are_periodic_and_deterministic():
    for B in (8000, 12500, 60000):
        for x in (se.clipping_station(B, 3, -1), se.dc_station(B, 3, 0.4), se.dc_station(B, 3, -0.4, stereo=True)):
            assert x.dtype == np.complex128 and x.shape == (B,)
            d = np.angle(x[0] * np.conj(x[-1])) / np.pi          # the step across the buffer's end is one of the signal's
            assert abs(d) <= se.STEP_BOUND
        assert np.array_equal(se.clipping_station(B, 3, 1), se.clipping_station(B, 3, 1))
    assert abs(np.mean(se.steps(se.dc_station(60000, 1, 0.4))) - 0.4) < 1e-3


def test_wideband_from_places_a_station_where_the_tuner_finds_it():
    N, B, C = 1_000_000, 12500, 3
    ref = se.oracle_tuner(B, C, N)
    st = [se.dc_station(B, i, 0.4) for i in range(C)]
    ref.load(se.wideband_from(st, N, ref.input_frequency, se.centres_of(B, C), B, gain=[0.3, 0.1, 0.2]))
    for i, g in enumerate((0.3, 0.1, 0.2)):
        iq = ref.run_pruned(i)
        assert np.max(np.abs(iq - g * st[i])) <= 2e-3 * g, i     # the Tuner's Hann weight is within 1e-3 of 1 here
