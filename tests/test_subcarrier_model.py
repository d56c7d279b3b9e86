"""CPU: the subcarrier tap's model (tests/subcarrier_model.py) -- every float32 yardstick the GPU test derives its bounds
from is evaluated here and lies below its pinned constant, the inputs keep the discriminator well conditioned, the
vectorised truth is the literal definition -- and what needs no device of the library: rcfm_subcarrier_create's argument
errors, and rcfm_subcarrier_describe, by which the case table is held to every tile the kernel can take.
"""

import ctypes
import inspect
import re

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


LDS_WIDE, LDS_MAX = 32 * 1024, 64 * 1024        # csrc/subcarrier.h: kTapWideLds (tiles of J > 256), kTapMaxLds
TILES = {0, 4, 8, 16, 32, 64, 128, 256, 512, 1024}


def describe(D, T):
    """(J, rpad, Q, lds_bytes) of rcfm_subcarrier_describe."""
    from radiocore._internal import hip
    J, rpad, Q, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    assert hip.lib().rcfm_subcarrier_describe(D, T, ctypes.byref(J), ctypes.byref(rpad), ctypes.byref(Q), ctypes.byref(lds)) == 0
    return J.value, rpad.value, Q.value, lds.value


def test_the_cases_reach_every_tile():
    """Every outcome of tap_tile (csrc/subcarrier.h) is run by a case, both neighbours of the last tile that fits are, and
    each case's comment names the J the library reports: a table that changes there shows here which case to add."""
    source = inspect.getsource(sm).splitlines()
    named = [(repr(case), case[0] // case[1], case[3]) for case in sm.CASES]
    named.append((repr(sm.RDS_TAP), rds_model.B // sm.RDS_TAP[0], sm.RDS_TAP[2]))
    named += [(repr(band), band[1] // band[2], band[4]) for band in (sm.PRIME_BAND, sm.PHASE_BAND_ONE, sm.PHASE_BAND_TWO)]
    seen = {}
    for text, D, T in named:
        J, rpad, Q, lds = describe(D, T)
        print("%s: D = %d, T = %d -> J = %d, rpad = %d, Q = %d, %d bytes of LDS" % (text, D, T, J, rpad, Q, lds))
        lines = [ln for ln in source if text in ln and "#" in ln]
        assert len(lines) == 1, text
        comment = lines[0].split("#", 1)[1]
        assert re.findall(r"\bJ = (\d+)\b", comment) == [str(J)], (text, J, comment)
        assert rpad == ((T + D - 1) // D + 3) // 4 * 4
        if J:
            assert Q == J + rpad + 4 and lds == 4 * D * Q
            assert lds <= (LDS_WIDE if J > 256 else LDS_MAX), (text, J, lds)
        else:
            assert Q == 0 and lds == 0
        seen.setdefault(J, []).append((D, T))
    assert set(seen) == TILES, sorted(TILES - set(seen))
    # the last D with a tile and the first without one, both at a T no longer than a row
    assert any(D == 1365 and T <= 1365 for D, T in seen[4]) and any(D == 1366 and T <= 1365 for D, T in seen[0])
    # with T <= D every polyphase row holds one tap: 1365 rows of 12 floats are the last that fit 64 KiB
    assert describe(1365, 1365)[0] == 4 and describe(1366, 1365)[0] == 0


def test_describe_refuses_what_create_refuses():
    from radiocore._internal import hip
    lib = hip.lib()
    J, rpad, Q, lds = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int(7), ctypes.c_int64(7)
    out = (ctypes.byref(J), ctypes.byref(rpad), ctypes.byref(Q), ctypes.byref(lds))
    for what, D, T in (("D < 1", 0, 3), ("negative D", -5, 3), ("even T", 25, 240), ("no taps", 25, 0), ("too many taps", 25, 4097),
                       ("negative T", 25, -1)):
        assert lib.rcfm_subcarrier_describe(D, T, *out) == -4, what
        assert lib.rcfm_last_error(), what
    assert (J.value, rpad.value, Q.value, lds.value) == (7, 7, 7, 7)
    assert lib.rcfm_subcarrier_describe(25, 241, None, out[1], out[2], out[3]) == -4
    assert lib.rcfm_subcarrier_describe(25, 241, out[0], out[1], out[2], None) == -4
    assert describe(25, 241) == (256, 12, 272, 27200)          # RDS (27.2 KB)
    assert describe(1, 4095) == (1024, 4096, 5124, 20496)      # the deepest row
    assert describe(2 ** 31 - 1, 1) == (0, 4, 0, 0) and describe(2 ** 31 - 1, 4095) == (0, 4, 0, 0)    # T + D - 1 beyond 32 bits


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
    for name, band, pinned in (("phase band one", sm.PHASE_BAND_ONE, sm.PHASE_BAND_ONE_YARDSTICK),
                               ("phase band two", sm.PHASE_BAND_TWO, sm.PHASE_BAND_TWO_YARDSTICK)):
        n, B, R, f, T = band
        ref, low = sm.small_band_channels(n, B)
        assert np.max(np.abs(sm.discriminator(ref))) <= signal_edges.STEP_BOUND
        err = pm.row_errors(sm.f32(low, R, f, sm.taps(T)), sm.small_band_truth(band))
        print("%s: float32 per channel %s, pinned %.3g, device bound %.3g" % (name, err, pinned, pm.gpu_bound(pinned)))
        assert pinned / 2.5 <= np.max(err) <= pinned
        assert np.all(np.max(np.abs(sm.small_band_truth(band)), axis=1) > 0)


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
