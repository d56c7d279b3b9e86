"""CPU: the reference, inputs, form predicate and tolerances of tests/tuner_model.py.

    reference    ref_channel is oracle.Tuner.run (np.roll + the full-length window, literally) and the closed-form
                 statement with the signed offset and delta, on every case and roll
    forms        the table reaches every form, from the library's own plans (rcfm_fft_describe) and the halo rule
    inputs       each named defect of a kernel moves at least one case by more than 10 x the GPU bound
    tolerances   the float32 / complex64 CPU evaluation of every case stays below YARDSTICK["tuner_run"], scipy.fft's
                 complex64 forward transform below YARDSTICK_FFT -- the device is held to gpu_bound() of them, which
                 nothing measured on a device enters
"""

import numpy as np
import pytest

import fft_model
import primitives_model as pm
import tuner_model as tm

pytest.importorskip("scipy.fft")

F64 = 1e-12          # float64 against float64: two statements of one sum
SMALL = [(n, B) for n, B in sorted(set(tm.cases())) if n <= tm.SMALL_N]


def _rows(fn, X, n, B, *a):
    return np.array([fn(X, n, r, B, *a) for r in tm.rolls(n, B)])


# ---- the table ---------------------------------------------------------------------------------------------------------------

def test_rolls_are_an_odd_count_and_reach_both_halos_and_the_band_edge():
    for n, B in tm.cases():
        r = tm.rolls(n, B)
        assert len(r) % 2 == 1 and all(0 <= v < n for v in r)
        base = [(n - v) % n for v in r]
        assert n - 3 in base and 5 in base and 0 in base
        assert {n - n // 2, n - n // 2 - 1} <= set(base)                  # centred on +-n / 2
        assert (B // 2) % n in base and (n - B // 2 - 1) % n in base          # the channel's own edges on bin 0
    x = tm.noise(10125)
    assert x.dtype == np.complex64 and not x.flags.writeable and tm.noise(10125) is x
    assert abs(float(np.mean(np.abs(x) ** 2)) - 2.0) < 0.1


def _forms():
    out = {}
    for n, bws in tm.TUNERS:
        halo = tm.tuner_halo(n, bws)
        for B in bws:
            out[(n, bws, B)] = (tm.gather_form(n, halo, B, fft_model.describe(B) is not None, fft_model.describe(n) is not None),
                                tm.nyquist_mode(n, B))
    return out


def test_the_table_reaches_every_form_by_the_librarys_own_plans():
    """The same coverage tests/test_hip_tuner_gather.py asserts from the handles' reported halos; here from tuner_halo."""
    forms = _forms()
    reached = {(n % 2, f, m) for (n, _, _), (f, m) in forms.items()}
    for parity in (0, 1):
        assert {(parity, "fast", "down"), (parity, "fast", "none")} <= reached, reached
    kinds = {(f, m) for f, m in forms.values()}
    assert {("general", "down"), ("general", "none"), ("tables", "down"), ("tables", "none")} <= kinds
    assert all(forms[(n, bws, B)] == ("general", "none") for n, bws in tm.TUNERS for B in bws if B == n)
    assert any(B == n and n % 2 == 0 for n, bws in tm.TUNERS for B in bws)
    assert forms[(10125, (1,), 1)] == ("tables", "none") and forms[(10125, (2,), 2)] == ("tables", "none")
    # both sides of the series limit, with nothing else different
    big = tm.TUNERS[0]
    assert tm.series_argument(10125, 800) < tm.SERIES_LIMIT <= tm.series_argument(10125, 810)
    assert forms[(big[0], big[1], 800)][0] == "fast" and forms[(big[0], big[1], 810)][0] == "general"
    assert {fft_model.describe(n) is not None for n, _ in tm.TUNERS} == {True, False}
    assert fft_model.describe(10007) is None


def test_halo_rule():
    assert tm.tuner_halo(10125, (675, 2250)) == 1136 and tm.tuner_halo(10125, (1,)) == 16
    assert tm.tuner_halo(10240, (10240, 640)) == 0 and tm.tuner_halo(10125, (10125,)) == 0     # would exceed n / 2
    assert tm.tuner_halo(*tm.HALO_EDGE) == 5120 and tm.tuner_halo(10240, (10238,)) == 0           # n / 2 itself is kept
    for n, bws in tm.TUNERS:
        assert 2 * tm.tuner_halo(n, bws) <= n


# ---- the reference -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,B", SMALL)
def test_reference_is_the_literal_roll_and_window_and_the_closed_form(n, B):
    X = tm.f32_spectrum(n)
    ref = tm.ref_channels(X, n, B)
    assert ref.dtype == np.complex128 and ref.shape == (len(tm.rolls(n, B)), B)
    literal = tm.worst_channel(_rows(tm.literal_channel, X, n, B), ref)
    closed = tm.worst_channel(_rows(tm.model_channel, X, n, B), ref)
    print("n=%d B=%d: oracle.Tuner.run %.3g, closed form %.3g" % (n, B, literal, closed))
    assert literal < F64 and closed < F64


def test_closed_form_at_the_large_size():
    n = 1_200_000
    X = tm.f32_spectrum(n)
    for B in (24000, 375000):
        assert tm.worst_channel(_rows(tm.model_channel, X, n, B), tm.ref_channels(X, n, B)) < F64


def test_reference_of_the_input_is_shared_and_read_only():
    y = tm.ref_channels_of_input(10007, 600)
    assert tm.ref_channels_of_input(10007, 600) is y and not y.flags.writeable
    assert tm.worst_channel(tm.ref_channels(tm.spectrum64(10007), 10007, 600), y) == 0.0


# ---- the inputs can see the defects ------------------------------------------------------------------------------------------

ASSERTED = tuple(d for d in tm.DEFECTS if d != "series c2 off by 10 %")


def test_each_defect_moves_a_case_by_more_than_ten_gpu_bounds():
    """A wrong t^2 coefficient of the series (c2) acts at the top of the series' range only: off by 10 % it is 3.0e-6 at
    (10125, 800), about two GPU bounds -- printed, not asserted; missing altogether it is 3.0e-5 there and nothing the
    bound could see at B = 600."""
    need = 10.0 * pm.gpu_bound(tm.YARDSTICK["tuner_run"])
    worst = {d: (0.0, None) for d in tm.DEFECTS}
    for n, B in sorted(set(tm.cases())):
        X = tm.f32_spectrum(n)
        ref = tm.ref_channels(X, n, B)
        for d in tm.DEFECTS:
            e = tm.worst_channel(_rows(tm.model_channel, X, n, B, d), ref)
            if e > worst[d][0]:
                worst[d] = (e, (n, B))
            if (d, n, B) in (("no delta", 10125, 675), ("no merge", 1_200_000, 24000), ("series c2 missing", 10125, 800),
                             ("series c2 missing", 10125, 600), ("series c2 off by 10 %", 10125, 800)):
                print("%s at n=%d B=%d: %.3g" % (d, n, B, e))
            if d == "no delta" and n % 2 == 0 or d == "no merge" and tm.nyquist_mode(n, B) == "none":
                assert e < F64, (d, n, B, e)                     # ... and where the defect cannot act, it does not
    for d in tm.DEFECTS:
        print("%-24s worst %.3g at %s (10 x the GPU bound: %.3g)" % (d, worst[d][0], worst[d][1], need))
    for d in ASSERTED:
        assert worst[d][0] > need, (d, worst[d])


def test_the_odd_fast_cases_see_a_missing_delta():
    """What no fixture before this table did: the fast form's delta on an odd n."""
    need = 10.0 * pm.gpu_bound(tm.YARDSTICK["tuner_run"])
    X = tm.f32_spectrum(10125)
    for B in (675, 600):
        e = tm.worst_channel(_rows(tm.model_channel, X, 10125, B, "no delta"), tm.ref_channels(X, 10125, B))
        assert e > need, (B, e)


# ---- tolerances ------------------------------------------------------------------------------------------------------------------

def test_gpu_bounds_reuse_the_primitives_rule():
    import conftest
    for v in (tm.YARDSTICK["tuner_run"], tm.YARDSTICK["tuner_run"] + tm.YARDSTICK_FFT):
        assert pm.gpu_bound(v) == 4 * v < conftest.TOL


@pytest.mark.parametrize("n,B", sorted(set(tm.cases())))
def test_yardstick_tuner_run(n, B):
    X = tm.f32_spectrum(n)
    got = _rows(tm.f32_channel, X, n, B)
    assert got.dtype == np.complex64
    worst = tm.worst_channel(got, tm.ref_channels(X, n, B))
    print("float32 tuner_run n=%d B=%d: %.3g" % (n, B, worst))
    assert worst < tm.YARDSTICK["tuner_run"]


@pytest.mark.parametrize("n", sorted({n for n, _ in tm.TUNERS}))
def test_yardstick_forward_fft(n):
    X = tm.spectrum64(n)
    worst = float(np.max(np.abs(tm.f32_spectrum(n) - X)) / np.max(np.abs(X)))
    print("float32 forward FFT n=%d: %.3g" % (n, worst))
    assert worst < tm.YARDSTICK_FFT
