"""CPU: the subcarrier tap's model (tests/subcarrier_model.py) -- every float32 yardstick the GPU test derives its bounds
from is evaluated here and lies below its pinned constant, the inputs keep the discriminator well conditioned, the
vectorised truth is the literal definition -- and rcfm_subcarrier_create's argument errors, which need no device.
"""

import ctypes

import numpy as np
import pytest

import primitives_model as pm
import rds_model
import signal_edges
import subcarrier_model as sm


@pytest.mark.parametrize("case", list(sm.CASES), ids=lambda c: "B%d-R%d-f%d-T%d" % c)
def test_float32_yardstick_of_every_case(case):
    B, R, f, T = case
    x, h = sm.case_input(B), sm.taps(T)
    assert x.shape == (sm.ROWS, B) and x.dtype == np.complex64
    ref = sm.truth(x, R, f, h)
    err = pm.worst_row(sm.f32(x, R, f, h), ref)
    print("B = %d, R = %d, f = %d, T = %d: float32 %.3g, pinned %.3g, device bound %.3g"
          % (B, R, f, T, err, sm.CASES[case], pm.gpu_bound(sm.CASES[case])))
    assert err <= sm.CASES[case]
    assert err >= sm.CASES[case] / 2.5, "the pinned constant is far above what float32 gives: re-measure it"
    assert np.all(np.max(np.abs(ref), axis=1) > 0)


@pytest.mark.parametrize("B", sorted({c[0] for c in sm.CASES}))
def test_inputs_keep_the_discriminator_conditioned(B):
    """The discriminator is discontinuous at +-1: no case may come close, or a flipped wrap could hide in the bound."""
    assert np.max(np.abs(sm.discriminator(sm.case_input(B)))) <= signal_edges.STEP_BOUND


def test_tuner_cases_yardsticks_and_conditioning():
    R, f, T, cutoff = sm.RDS_TAP
    ref, low = sm.rds_channels()
    assert np.max(np.abs(sm.discriminator(ref))) <= signal_edges.STEP_BOUND
    err = pm.row_errors(sm.f32(low, R, f, sm.rds_taps(rds_model.B, R, T, cutoff)), sm.rds_truth())
    print("RDS band: float32 per channel", err, "pinned", sm.RDS_YARDSTICK)
    for e, pinned in zip(err, sm.RDS_YARDSTICK):
        assert pinned / 2.5 <= e <= pinned
    n, B, R, f, T = sm.PRIME_BAND
    ref, low = sm.prime_band_channels()
    assert np.max(np.abs(sm.discriminator(ref))) <= signal_edges.STEP_BOUND
    err = pm.worst_row(sm.f32(low, R, f, sm.taps(T)), sm.truth(ref, R, f, sm.taps(T)))
    print("prime band: float32 %.3g, pinned %.3g" % (err, sm.PRIME_BAND_YARDSTICK))
    assert sm.PRIME_BAND_YARDSTICK / 2.5 <= err <= sm.PRIME_BAND_YARDSTICK


def test_truth_is_the_literal_double_loop():
    B, R, f, T = 1000, 200, -300, 31
    x, h = sm.case_input(B), sm.taps(T)
    want = sm.truth_loops(x, R, f, h)
    assert np.max(np.abs(sm.truth(x, R, f, h) - want)) <= 1e-14 * np.max(np.abs(want))


def test_identity_case_is_the_discriminator():
    B, R, f, T = 6000, 6000, 0, 1
    assert np.array_equal(sm.taps(T), np.ones(1, np.float32))
    y = sm.truth(sm.case_input(B), R, f, sm.taps(T))
    want = np.array([signal_edges.steps(row) for row in sm.case_input(B)])
    assert np.array_equal(y.real, want) and not np.any(y.imag)


def test_a_subcarrier_comes_out_at_deviation_over_rate():
    """include/rcfm.h: a subcarrier at f with deviation Delta Hz and phase phi comes out as (Delta / B) sum(h) e^{i phi}."""
    B, R, f, T = 12500, 500, 1000, 151
    delta, phi = 40.0, 0.7
    h = sm.rds_taps(B, R, T, 100.0)                                 # the image at -f lands at 2 f, far in the stop band
    n = np.arange(B)
    d = 2.0 * delta / B * np.cos(2 * np.pi * f * n / B + phi)        # phase step / pi of a tone with `delta` Hz deviation
    x = np.exp(1j * np.pi * np.cumsum(d)).astype(np.complex64)
    y = sm.truth(x, R, f, h)[0]
    want = delta / B * float(np.sum(h.astype(np.float64))) * np.exp(1j * phi)
    assert np.max(np.abs(y[10:-10] - want)) < 5e-3 * abs(want)


def test_argument_errors_need_no_device():
    from radiocore._internal import hip
    lib = hip.lib()
    taps = np.ones(3, np.float32)
    fp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    out = ctypes.c_void_p()

    def create(C=1, B=1000, R=100, f=10, t=fp, nt=3, chunk=0, o=ctypes.byref(out)):
        return lib.rcfm_subcarrier_create(C, B, R, f, t, nt, chunk, o)

    bad = np.array([1.0, np.nan, 1.0], np.float32)
    for what, status in (("even ntaps", create(nt=2)), ("no taps", create(nt=0)), ("too many taps", create(nt=4097)),
                         ("R does not divide B", create(R=300)), ("f beyond B / 2", create(f=501)),
                         ("-f beyond B / 2", create(f=-501)), ("NULL taps", create(t=None)), ("NULL out", create(o=None)),
                         ("C < 1", create(C=0)), ("B < 2", create(B=1, R=1, f=0)), ("R < 1", create(R=0)),
                         ("NaN tap", create(t=bad.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))):
        assert status == -4, what
        assert lib.rcfm_last_error(), what
    assert not out.value
    assert lib.rcfm_subcarrier_run(None, 1, None, None, None) == -4
    assert lib.rcfm_pipeline_subcarrier(None, None, 0, 1, None, None) == -4
    assert lib.rcfm_subcarrier_destroy(None) == 0
