"""GPU: the subcarrier tap (rcfm_subcarrier_*, rcfm_pipeline_subcarrier; radiocore.Subcarrier, Tuner.subcarrier) against
its definition in include/rcfm.h, evaluated in float64 by tests/subcarrier_model.py on the same complex64 input.

Bounds: max|delta| / max|truth| per channel, worst channel, within primitives_model.gpu_bound(yardstick) = min(4 x yardstick,
1e-4), the yardstick being the float32 CPU figure of the very case that tests/test_subcarrier_model.py pins.  Every case
prints its worst row and its bound.  Sub-ranges, streams and chunk sizes are compared bit for bit.
"""

import ctypes

import numpy as np
import pytest

import primitives_model as pm
import rds_model
import subcarrier_model as sm
from conftest import ROOT, have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ERR_SIZE, ERR_INDEX, ERR_STATE = -1, -2, -5


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def hip(rc):
    from radiocore._internal import hip
    return hip


def _truth(case):
    B, R, f, T = case
    if case not in _truth.cache:
        _truth.cache[case] = sm.truth(sm.case_input(B), R, f, sm.taps(T))
    return _truth.cache[case]


_truth.cache = {}


def _tile(hip, D, T):
    """J of rcfm_subcarrier_describe: the outputs per workgroup the kernel takes (0: the single-output kernel)."""
    J, rpad, Q, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    hip.check(hip.lib().rcfm_subcarrier_describe(D, T, ctypes.byref(J), ctypes.byref(rpad), ctypes.byref(Q), ctypes.byref(lds)))
    return J.value


def _segments(y, want, edge):
    """primitives_model.segment_errors (head, interior, tail) of complex rows in row_errors' metric, |delta| / max|truth|:
    the function takes real arrays, so it is given |truth| and |truth| + |delta|."""
    mag = np.abs(np.asarray(want, np.complex128))
    return pm.segment_errors(mag + np.abs(np.asarray(y, np.complex128) - want), mag, edge)


# ---- the standalone cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("case", list(sm.CASES), ids=lambda c: "B%d-R%d-f%d-T%d" % c)
def test_case_within_its_bound(rc, hip, case, batch):
    B, R, f, T = case
    x = sm.case_input(B)[:batch]
    tap = rc.Subcarrier(B, R, f, sm.taps(T), batch=batch)
    y = tap.run(x[0] if batch == 1 else x)
    assert y.dtype == np.complex64 and y.shape == ((R,) if batch == 1 else (batch, R))
    y, want = y.reshape(batch, R), _truth(case)[:batch]
    err = pm.row_errors(y, want)
    bound = pm.gpu_bound(sm.CASES[case])
    print("B = %d, R = %d, f = %d, T = %d (J = %d), batch %d: worst row %d at %.3g, bound %.3g"
          % (B, R, f, T, _tile(hip, B // R, T), batch, int(np.argmax(err)), float(np.max(err)), bound))
    assert np.max(err) <= bound
    if case in sm.EDGE_CASES:
        # the outputs whose taps reach beyond the row (zero extension, d[0] = 0) apart from the interior, each against the
        # whole row's peak: what the staging does at a row's ends is not read off a figure the interior dominates
        edge = sm.edge_outputs(B, R, T)
        assert 0 < edge and 2 * edge < R
        head, interior, tail = _segments(y, want, edge)
        print("    %d outputs at either row end: head %.3g, tail %.3g; interior %.3g" % (edge, head, tail, interior))
        assert head <= bound and tail <= bound
        assert interior <= bound


def _raw_run(hip, handle, x_dev, count, R, stream=None):
    import torch
    y = torch.full((count, R), float("nan"), dtype=torch.complex64, device="cuda")
    hip.check(hip.lib().rcfm_subcarrier_run(handle.value, count, hip.ptr(x_dev), hip.ptr(y),
                                            stream if stream is not None else hip.stream()))
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("case", [(240000, 9600, 57000, 241), (1001, 91, 77, 15), (6000, 240, 2999, 257), (6000, 1, 1234, 4095),
                                  (12500, 125, 1000, 241), (27300, 20, 9000, 241), (12000, 6000, 1500, 4095)],   # J = 128, J = 4, deep rows
                         ids=lambda c: "B%d-R%d-f%d-T%d" % c)
def test_sub_range_stream_and_chunk_are_bit_identical(rc, hip, case):
    import torch
    B, R, f, T = case
    x = hip.to_device(sm.case_input(B).copy())
    whole = rc.Subcarrier(B, R, f, sm.taps(T), batch=3)
    y = _raw_run(hip, whole._handle, x, 3, R)
    assert not np.any(np.isnan(y.real))
    # rows 1 - 2 alone, count = 2
    alone = _raw_run(hip, whole._handle, x[1:], 2, R)
    assert np.array_equal(alone.view(np.uint32), y[1:].view(np.uint32))
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    again = _raw_run(hip, whole._handle, x, 3, R, ctypes.c_void_p(side.cuda_stream))
    assert np.array_equal(again.view(np.uint32), y.view(np.uint32))
    # one channel per launch
    single = rc.Subcarrier(B, R, f, sm.taps(T), batch=3, chunk=1)
    assert np.array_equal(_raw_run(hip, single._handle, x, 3, R).view(np.uint32), y.view(np.uint32))
    # more channels than the handle was created for
    assert hip.lib().rcfm_subcarrier_run(single._handle.value, 4, hip.ptr(x), hip.ptr(x), hip.stream()) == ERR_INDEX


def test_constructor_refuses_what_the_library_would(rc):
    for kw in (dict(taps=np.ones(4)), dict(output_size=7), dict(frequency=501), dict(frequency=10.5), dict(taps=[1.0, np.inf, 1.0]),
               dict(batch=0), dict(taps=np.ones(4097))):
        args = dict(input_size=1000, output_size=100, frequency=10, taps=np.ones(3))
        args.update(kw)
        with pytest.raises(ValueError):
            rc.Subcarrier(**args)
    tap = rc.Subcarrier(1000, 100, 10, np.ones(3))
    with pytest.raises(ValueError, match="mismatch"):
        tap.run(np.zeros(999, np.complex64))


# ---- through the Tuner ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rds_tuner(rc):
    tuner = rc.Tuner()
    for fc in rds_model.CENTRES:
        tuner.add_channel(fc, rds_model.B, rc.WBFM(rds_model.B, 48000))
    tuner.request_bandwidth(float(rds_model.N))
    assert tuner.input_frequency == rds_model.input_frequency()
    R, f, T, cutoff = sm.RDS_TAP
    from radiocore.tools import rds
    tap = rc.Subcarrier(rds_model.B, R, f, rds.taps(rds_model.B, R, T, cutoff))
    return tuner, tap


def test_tuner_refuses_before_a_load(rc, hip, rds_tuner):
    tuner, tap = rds_tuner
    fresh = rc.Tuner()
    for fc in rds_model.CENTRES:
        fresh.add_channel(fc, rds_model.B, rc.WBFM(rds_model.B, 48000))
    with pytest.raises(RuntimeError):
        fresh.subcarrier(tap)
    handle = fresh._device_tuner(rds_model.N)
    import torch
    out = torch.zeros((3, sm.RDS_TAP[0]), dtype=torch.complex64, device="cuda")
    lib = hip.lib()
    batched = tap._create(3, 0)
    assert lib.rcfm_pipeline_subcarrier(handle, batched.value, 0, 3, hip.ptr(out), hip.stream()) == ERR_STATE
    assert b"rcfm_pipeline_subcarrier" in lib.rcfm_last_error()
    assert lib.rcfm_pipeline_subcarrier(handle, batched.value, 2, 2, hip.ptr(out), hip.stream()) == ERR_INDEX
    assert lib.rcfm_pipeline_subcarrier(handle, tap._handle.value, 0, 3, hip.ptr(out), hip.stream()) == ERR_INDEX   # a handle for one channel


def test_rds_band_through_the_tuner(rc, rds_tuner):
    from radiocore.tools import rds
    tuner, tap = rds_tuner
    R = sm.RDS_TAP[0]
    tuner.load(rds_model.band().copy())
    before = tuner.run_all()
    y = tuner.subcarrier(tap)
    tuner.reset_states()                              # (WBFM carries de-emphasis state from call to call)
    assert np.array_equal(tuner.run_all(), before)    # the same audio before and after the tap call
    third = tuner.run_all()                           # ... and the state goes on as if the tap had never run (below)
    assert y.dtype == np.complex64 and y.shape == (3, R)
    err = pm.row_errors(y, sm.rds_truth())
    for k, (e, yard) in enumerate(zip(err, sm.RDS_YARDSTICK)):
        print("station %d: %.3g, bound %.3g" % (k, e, pm.gpu_bound(yard)))
    for e, yard in zip(err, sm.RDS_YARDSTICK):
        assert e <= pm.gpu_bound(yard)
    for k, (pi, ps) in enumerate(rds_model.STATIONS):
        found = rds.groups(rds.bits(y[k], R))
        print("station %d: %d groups, PI %04X, PS %r" % (k, len(found), rds.station(found)[0] or 0, rds.station(found)[1]))
        assert len(found) >= 8 and rds.station(found) == (pi, ps)
    # a sub-range is bit-identical to those rows of the full range, and so is a second call
    part = tuner.subcarrier(tap, first=1, count=2)
    assert np.array_equal(part.view(np.uint32), y[1:3].view(np.uint32))
    assert np.array_equal(tuner.subcarrier(tap).view(np.uint32), y.view(np.uint32))
    assert len(tuner._taps) == 1                      # one batched handle per (B, R, f, taps)
    # a tap for another channel width
    other = rc.Subcarrier(120000, 4800, 57000, rds.taps(120000, 4800, cutoff=2000.0))
    with pytest.raises(ValueError, match="mismatch"):
        tuner.subcarrier(other)
    with pytest.raises(IndexError):
        tuner.subcarrier(tap, first=2, count=2)
    # the tap touches no demodulator workspace or state: a twin tuner that never runs the tap gives the same audio for
    # the same buffer twice in a row
    twin = rc.Tuner()
    for fc in rds_model.CENTRES:
        twin.add_channel(fc, rds_model.B, rc.WBFM(rds_model.B, 48000))
    twin.request_bandwidth(float(rds_model.N))
    twin.load(rds_model.band().copy())
    assert np.array_equal(twin.run_all(), before)
    assert np.array_equal(twin.run_all(), third)


def test_band_without_phase_output(rc, hip):
    """B = 3001 is prime: the Tuner's inverse FFT of these channels is rocFFT's, which hands over samples, not phases."""
    n, B, R, f, T = sm.PRIME_BAND
    plan = hip.FftPlan()
    assert hip.lib().rcfm_fft_describe(B, 0, ctypes.byref(plan)) != 0, "the engine has a plan for this length now: pick another"
    x, f_in, centres = sm.prime_band()
    tuner = rc.Tuner()
    for fc in centres:
        tuner.add_channel(fc, B, rc.FM(B, 1001))
    tuner.request_bandwidth(float(n))
    assert tuner.input_frequency == f_in
    tuner.load(x.copy())
    tap = rc.Subcarrier(B, R, f, sm.taps(T))
    y = tuner.subcarrier(tap)
    want = sm.truth(sm.prime_band_channels()[0], R, f, sm.taps(T))
    err = pm.row_errors(y, want)
    bound = pm.gpu_bound(sm.PRIME_BAND_YARDSTICK)
    print("prime band: worst channel %d at %.3g, bound %.3g" % (int(np.argmax(err)), float(np.max(err)), bound))
    assert np.max(err) <= bound
    # the from-samples form on the Tuner's own channel samples is the same kernel on the same input
    iq = tuner.run_channels(0, 3)
    direct = rc.Subcarrier(B, R, f, sm.taps(T), batch=3).run(iq)
    assert np.array_equal(direct.view(np.uint32), y.view(np.uint32))


# ---- the from-phase form beyond RDS, the pipeline's chunk loop, shard ---------------------------------------------------------------

PHASE_BANDS = {"one": (sm.PHASE_BAND_ONE, sm.PHASE_BAND_ONE_YARDSTICK), "two": (sm.PHASE_BAND_TWO, sm.PHASE_BAND_TWO_YARDSTICK)}


def _phase_band_tuner(rc, hip, band):
    """A Tuner over sm.small_band of `band`, not loaded; the engine plans B, so its channels are handed over as phases."""
    n, B, R, f, T = band
    plan = hip.FftPlan()
    assert hip.lib().rcfm_fft_describe(B, 0, ctypes.byref(plan)) == 0, "the engine lost its plan for this length: pick another"
    x, f_in, centres = sm.small_band(n, B)
    tuner = rc.Tuner()
    for fc in centres:
        tuner.add_channel(fc, B, rc.FM(B, B // 5))
    tuner.request_bandwidth(float(n))
    assert tuner.input_frequency == f_in
    return tuner


@pytest.mark.parametrize("name", list(PHASE_BANDS))
def test_band_with_phase_output(rc, hip, name):
    """k_subcarrier_tap<true> at tiles other than RDS's: band one with 16-byte phase rows (J = 128), band two with an odd
    B, whose phase rows are only 4-byte aligned (J = 64, scalar loads)."""
    band, yardstick = PHASE_BANDS[name]
    n, B, R, f, T = band
    tuner = _phase_band_tuner(rc, hip, band)
    tuner.load(sm.small_band(n, B)[0].copy())
    tap = rc.Subcarrier(B, R, f, sm.taps(T))
    y = tuner.subcarrier(tap)
    assert y.dtype == np.complex64 and y.shape == (3, R)
    want = sm.small_band_truth(band)
    bound = pm.gpu_bound(yardstick)
    err = pm.row_errors(y, want)
    # the from-samples form on the Tuner's own channel samples: another kernel instance on another input (the samples
    # instead of their phases), so within the bound of the truth, not bit for bit
    direct = rc.Subcarrier(B, R, f, sm.taps(T), batch=3).run(tuner.run_channels(0, 3))
    err_direct = pm.row_errors(direct, want)
    for k in range(3):
        print("phase band %s (B = %d, R = %d, f = %d, T = %d, J = %d), channel %d: from phases %.3g, from samples %.3g, bound %.3g"
              % (name, B, R, f, T, _tile(hip, B // R, T), k, err[k], err_direct[k], bound))
    assert np.all(err <= bound)
    assert np.all(err_direct <= bound)


def _rds_setup(rc, hip):
    from radiocore.tools import rds
    R, f, T, cutoff = sm.RDS_TAP

    def make():
        tuner = rc.Tuner()
        for fc in rds_model.CENTRES:
            tuner.add_channel(fc, rds_model.B, rc.WBFM(rds_model.B, 48000))
        tuner.request_bandwidth(float(rds_model.N))
        return tuner

    return make, rc.Subcarrier(rds_model.B, R, f, rds.taps(rds_model.B, R, T, cutoff)), rds_model.band(), R


def _band_one_setup(rc, hip):
    n, B, R, f, T = sm.PHASE_BAND_ONE
    return (lambda: _phase_band_tuner(rc, hip, sm.PHASE_BAND_ONE)), rc.Subcarrier(B, R, f, sm.taps(T)), sm.small_band(n, B)[0], R


TAPPED_BANDS = {"rds": _rds_setup, "one": _band_one_setup}


@pytest.mark.parametrize("name", list(TAPPED_BANDS))
def test_pipeline_chunks_are_bit_identical(rc, hip, name):
    """rcfm_pipeline_subcarrier with a handle whose chunk is below the count: several rounds of the Tuner's inverse FFT and
    the tap kernel through ONE workspace, one channel (chunk 1) and two plus one (chunk 2) at a time."""
    import torch
    make, tap, x, R = TAPPED_BANDS[name](rc, hip)
    tuner = make()
    tuner.load(x.copy())
    y = tuner.subcarrier(tap)                        # the Tuner's own handle: chunk 0, all three channels in one round
    assert y.shape == (3, R) and np.all(np.isfinite(y.view(np.float32)))
    handle = tuner._ready()
    for chunk in (1, 2):
        batched = tap._create(3, chunk)
        out = torch.full((3, R), float("nan"), dtype=torch.complex64, device="cuda")
        hip.check(hip.lib().rcfm_pipeline_subcarrier(handle, batched.value, 0, 3, hip.ptr(out), hip.stream()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert not np.any(np.isnan(got.view(np.float32))), chunk
        assert np.array_equal(got.view(np.uint32), y.view(np.uint32)), chunk
        # a sub-range that starts inside the handle's second round
        out.fill_(float("nan"))
        hip.check(hip.lib().rcfm_pipeline_subcarrier(handle, batched.value, 1, 2, hip.ptr(out), hip.stream()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:2].view(np.uint32), y[1:].view(np.uint32)), chunk
        assert np.all(np.isnan(got[2].real)), chunk                    # nothing is written beyond `count` rows (NaN + 0j)


@pytest.mark.parametrize("name", list(TAPPED_BANDS))
def test_tap_after_shard(rc, hip, name):
    """After shard(1, 2) and a fresh load the spectrum holds the bins of channels 1 - 2 only: the tap of those two is that
    of the whole load bit for bit, channel 0 is refused by the library, and the audio is that of a tuner never tapped."""
    make, tap, x, R = TAPPED_BANDS[name](rc, hip)
    tuner = make()
    tuner.load(x.copy())
    y = tuner.subcarrier(tap)
    tuner.shard(1, 2)
    tuner.load(x.copy())
    part = tuner.subcarrier(tap)
    assert part.dtype == np.complex64 and part.shape == (2, R)
    assert np.array_equal(part.view(np.uint32), y[1:3].view(np.uint32))
    with pytest.raises(RuntimeError, match="shard"):
        tuner.subcarrier(tap, first=0, count=1)
    assert np.array_equal(tuner.subcarrier(tap, first=2, count=1).view(np.uint32), y[2:3].view(np.uint32))
    audio = tuner.run_all()
    twin = make()
    twin.shard(1, 2)
    twin.load(x.copy())
    want = twin.run_all()
    assert audio.shape == want.shape and audio.shape[0] == 2
    assert np.array_equal(audio, want)


def test_tap_follows_a_growing_channel_list(rc):
    """A tap used before add_channel serves the longer list afterwards: the Tuner's batched handle is sized for all channels."""
    n, B, R, f, T = sm.PRIME_BAND
    x, f_in, centres = sm.prime_band()
    tuner = rc.Tuner()
    for fc in centres:
        tuner.add_channel(fc, B, rc.FM(B, 1001))
    tuner.request_bandwidth(float(n))
    tuner.load(x.copy())
    tap = rc.Subcarrier(B, R, f, sm.taps(T))
    want = sm.truth(sm.prime_band_channels()[0], R, f, sm.taps(T))
    bound = pm.gpu_bound(sm.PRIME_BAND_YARDSTICK)
    assert np.max(pm.row_errors(tuner.subcarrier(tap), want)) <= bound
    for fc in (1e6 + 6 * B, 1e6 - 6 * B):            # two empty channels, the band's centre stays where it was
        tuner.add_channel(fc, B, rc.FM(B, 1001))
    tuner.request_bandwidth(float(n))
    assert tuner.input_frequency == f_in
    tuner.load(x.copy())
    y = tuner.subcarrier(tap)
    assert y.shape == (5, R) and np.all(np.isfinite(y.view(np.float32)))
    err = pm.row_errors(y[:3], want)
    print("five channels: worst of the first three %.3g, bound %.3g" % (float(np.max(err)), bound))
    assert np.max(err) <= bound
    assert len(tuner._taps) == 1


def test_fm_rds_example():
    """examples/fm_rds.py names its three stations."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fm_rds", os.path.join(ROOT, "examples", "fm_rds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    audio, found = mod.run()
    assert audio.shape == (3, mod.AUDIO, 2)
    for (_, pi, ps), (got_pi, got_ps, groups) in zip(mod.STATIONS, found):
        print("PI %04X PS %r (%d groups)" % (got_pi or 0, got_ps, groups))
        assert (got_pi, got_ps) == (pi, ps) and groups >= 8
