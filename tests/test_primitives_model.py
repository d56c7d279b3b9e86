"""CPU: the references, inputs and tolerances of tests/primitives_model.py.

    references   against scipy, in float64, at the parities and directions tests/test_hip_primitives.py runs
    generators   rows distinct, amplitudes spread over three decades, phase steps bounded, Nyquist bins loaded
    tolerances   the float32 / complex64 CPU evaluation of every case stays below its YARDSTICK constant -- the device
                 is then held to gpu_bound() of that constant, which nothing measured on a device enters
"""

import numpy as np
import pytest

import primitives_model as pm
import radiocore_oracle as oracle

ss = pytest.importorskip("scipy.signal")

F64 = 1e-11          # float64 against float64: two implementations of one sum


# ---- references against scipy ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx,n,m", [(True, n, m) for n, m in pm.RESAMPLE_COMPLEX if n <= 10007] +
                         [(False, n, m) for n, m in pm.RESAMPLE_REAL if n <= 1001])
def test_resample_reference_is_scipy_resample_with_the_shifted_hamming_window(cplx, n, m):
    import scipy.fft
    x = pm.spectral_input(3, n, m, cplx, 1).astype(np.complex128 if cplx else np.float64)
    w = scipy.fft.fftshift(ss.get_window("hamm", n))
    want = np.array([ss.resample(row, m, window=w) for row in x])
    assert pm.worst_row(pm.ref_resample(x, m), want) < F64


@pytest.mark.parametrize("kind", ["firwin", "random"])
@pytest.mark.parametrize("ntaps", pm.FILTFILT_TAPS)
def test_filtfilt_reference_is_scipy_filtfilt_and_the_closed_form_holds_for_any_taps(kind, ntaps):
    b = pm.filter_taps(kind, ntaps)
    if kind == "random" and ntaps > 2:
        assert not np.allclose(b, b[::-1], atol=1e-3), "the drawn filter came out symmetric"
    assert abs(float(np.sum(b.astype(np.float64))) - 1.0) < 1e-6
    for n in pm.filtfilt_sizes(ntaps)[:3]:
        x = pm.filtfilt_input(3, n, 2).astype(np.float64)
        want = np.array([ss.filtfilt(b.astype(np.float64), [1.0], row) for row in x])
        ref = pm.ref_filtfilt(b, x)
        assert pm.worst_row(ref, want) < F64
        # what the kernel implements: g = b * reverse(b) over an odd extension by ntaps - 1
        closed = np.array([oracle.filtfilt_fir_closed_form(b, row) for row in x])
        assert pm.worst_row(closed, want) < F64
    with pytest.raises(ValueError, match="must be greater than padlen, which is %d" % (3 * ntaps)):
        pm.ref_filtfilt(b, np.ones((1, 3 * ntaps)))


@pytest.mark.parametrize("ntaps", pm.LFILTER_TAPS)
def test_lfilter_reference_is_scipy_lfilter_with_zi_over_consecutive_buffers(ntaps):
    b = pm.filter_taps("random", ntaps, seed=3)
    for n in pm.lfilter_sizes(ntaps):
        x, zi = pm.lfilter_input(3, n, ntaps, pm.LFILTER_BUFFERS, 4)
        state = zi.astype(np.float64)
        want_y, want_z = ss.lfilter(b.astype(np.float64), [1.0], np.concatenate(list(x.astype(np.float64)), axis=1),
                                    axis=1, zi=state) if ntaps > 1 else \
            (ss.lfilter(b.astype(np.float64), [1.0], np.concatenate(list(x.astype(np.float64)), axis=1), axis=1),
             np.zeros((3, 0)))
        for k in range(pm.LFILTER_BUFFERS):
            y, state = pm.ref_lfilter(b, x[k], state)
            assert pm.worst_row(y, want_y[:, k * n:(k + 1) * n]) < F64
        if ntaps > 1:
            assert pm.worst_row(state, want_z) < F64


@pytest.mark.parametrize("n", [16, 17, 6000, 10007])
def test_hilbert_reference_is_scipy_hilbert(n):
    x = pm.spectral_input(3, n, n, False, 5).astype(np.float64)
    assert pm.worst_row(pm.ref_hilbert(x), ss.hilbert(x, axis=1)) < F64


def test_discriminator_and_pll_references_are_what_they_say():
    iq = pm.discriminator_input(3, 257, 6)
    d = pm.ref_discriminator(iq)
    assert np.all(d[:, 0] == 0.0)
    z = iq.astype(np.complex128)
    assert np.allclose(d[:, 1:], np.diff(np.unwrap(np.angle(z), axis=1), axis=1) / np.pi, atol=1e-12)
    for mult in pm.PLL_INTEGER + pm.PLL_PRINCIPAL:
        zz = pm.pll_input(257, mult, 7).astype(np.complex128)
        u = zz / np.abs(zz)
        if mult in pm.PLL_INTEGER:          # the power itself, on the unit circle (no overflow in float64)
            assert np.allclose(pm.ref_pll(zz, mult, 0), np.real(u ** mult), atol=1e-12)
            assert np.allclose(pm.ref_pll(zz, mult, 1), np.imag(u ** mult), atol=1e-12)
        else:                               # numpy's complex128 power is the principal branch
            assert np.allclose(pm.ref_pll(zz, mult, 1), np.imag(u ** complex(mult)), atol=1e-10)


# ---- generators ------------------------------------------------------------------------------------------------------------

def _rows_distinct(x):
    x = np.asarray(x)
    unit = x / np.max(np.abs(x), axis=1, keepdims=True)       # distinct beyond their amplitude
    for a in range(len(x)):
        for b in range(a + 1, len(x)):
            if x.shape[1] > 1:
                assert np.max(np.abs(unit[a] - unit[b])) > 0.05, (a, b)
            else:
                assert x[a, 0] != x[b, 0]


@pytest.mark.parametrize("C", [2, 3, 5])
def test_rows_are_distinct_and_spread_over_three_decades(C):
    amps = pm.row_amplitudes(C)
    assert amps[0] == 1.0 and abs(amps[-1] - 1e-3) < 1e-12 and np.all(np.diff(amps) < 0)
    for x in (pm.spectral_input(C, 1000, 200, True, 1), pm.spectral_input(C, 1000, 200, False, 1),
              pm.noise_rows(C, 1024, 2), pm.ramp_rows(C, 1024), pm.filtfilt_input(C, 1024, 2),
              pm.lfilter_input(C, 51, 51, 3, 4)[0][1], pm.lfilter_input(C, 51, 51, 3, 4)[1],
              pm.discriminator_input(C, 257, 6)):
        _rows_distinct(x)
        rms = np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2, axis=1))
        assert 200.0 < rms[0] / rms[-1] < 5000.0, rms            # 1e3 within the scatter of a 50-sample draw


def test_discriminator_steps_are_bounded_and_the_row_boundary_is_not():
    for n in pm.DISC_SIZES:
        iq = pm.discriminator_input(3, n, 6)
        d = pm.ref_discriminator(iq)
        assert np.max(np.abs(d)) <= pm.STEP_BOUND + 1e-6
        flat = signal_edges_steps(iq.reshape(-1))                # what a difference across rows would see
        for c in (1, 2):
            assert abs(abs(flat[c * n]) - pm.ROW_STEP) < 1e-3, (n, c, flat[c * n])


def signal_edges_steps(z):
    import signal_edges
    return signal_edges.steps(z)


@pytest.mark.parametrize("cplx,n,m", [(True, n, m) for n, m in pm.RESAMPLE_COMPLEX] +
                         [(False, n, m) for n, m in pm.RESAMPLE_REAL] +
                         [(False, n, n) for n in pm.HILBERT_ENGINE_SIZES + pm.HILBERT_ROCFFT_SIZES + pm.HILBERT_SMALLEST])
def test_the_nyquist_bins_hold_their_share_of_every_row(cplx, n, m):
    share = pm.nyquist_share(pm.spectral_input(3, n, m, cplx, 1), m)
    assert np.all(share >= pm.NYQUIST_SHARE), share


def test_pll_magnitudes_keep_the_power_normal():
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    for mult in pm.PLL_INTEGER + pm.PLL_PRINCIPAL:
        lo, hi = pm.pll_magnitude_range(mult)
        a = np.abs(pm.pll_input(4099, mult, 7).astype(np.complex128))
        assert lo * 0.999 <= a.min() and a.max() <= hi * 1.001
        p = max(1.0, abs(mult))
        assert a.min() ** p > tiny * 2.0 ** 20 and a.max() ** p < huge / 2.0 ** 20
        if abs(mult) >= 1:
            for outside in (1, -1):
                q = np.abs(pm.pll_input(4099, mult, 7, outside).astype(np.complex128)) ** p
                assert np.all(q > huge * 2.0 ** 50) if outside > 0 else np.all(q < tiny / 2.0 ** 50)


# ---- tolerances: float32 on the CPU against the float64 reference, on the inputs of the GPU test ------------------------------

def test_gpu_bounds_are_four_yardsticks_and_never_looser_than_the_parity_tolerance():
    import conftest
    assert pm.TOL == conftest.TOL
    for key, v in pm.YARDSTICK.items():
        assert pm.gpu_bound(v) == min(4 * v, conftest.TOL) and pm.gpu_bound(v) <= conftest.TOL, key
    assert pm.gpu_bound(1.0) == conftest.TOL
    bounds = [pm.pll_gpu_bound(m) for m in pm.PLL_INTEGER]
    assert bounds == sorted(bounds) and bounds[-1] <= conftest.TOL


@pytest.mark.parametrize("cplx,n,m", [(True, n, m) for n, m in pm.RESAMPLE_COMPLEX] +
                         [(False, n, m) for n, m in pm.RESAMPLE_REAL])
def test_yardstick_resample(cplx, n, m):
    worst = 0.0
    for C in pm.BATCHES:
        x = pm.spectral_input(C, n, m, cplx, 1)
        worst = max(worst, pm.worst_row(pm.f32_resample(x, m), pm.ref_resample(x, m)))
    print("float32 resample %s %d -> %d: %.3g" % ("complex" if cplx else "real", n, m, worst))
    assert worst < pm.YARDSTICK["resample_complex" if cplx else "resample_real"]


@pytest.mark.parametrize("kind", ["firwin", "random"])
@pytest.mark.parametrize("ntaps", pm.FILTFILT_TAPS)
def test_yardstick_filtfilt(kind, ntaps):
    b = pm.filter_taps(kind, ntaps)
    worst = 0.0
    for n in pm.filtfilt_sizes(ntaps):
        for C in pm.FILTFILT_BATCHES:
            for x in (pm.filtfilt_input(C, n, 2), pm.ramp_rows(C, n)):
                worst = max(worst, pm.worst_row(pm.f32_filtfilt(b, x), pm.ref_filtfilt(b, x)))
        # unit DC gain and a symmetric g = b * reverse(b): the float64 reference returns a ramp as it went in
        r = pm.ramp_rows(4, n)
        assert pm.worst_row(pm.ref_filtfilt(b, r), r.astype(np.float64)) < 2e-7
    print("float32 filtfilt %s %d taps: %.3g" % (kind, ntaps, worst))
    assert worst < pm.YARDSTICK["filtfilt"]


@pytest.mark.parametrize("ntaps", pm.LFILTER_TAPS)
def test_yardstick_lfilter(ntaps):
    b = pm.filter_taps("random", ntaps, seed=3)
    worst_y = worst_z = 0.0
    for n, C in [(n, C) for n in pm.lfilter_sizes(ntaps) for C in pm.LFILTER_BATCHES]:
        x, zi = pm.lfilter_input(C, n, ntaps, pm.LFILTER_BUFFERS, 4)
        # two float32 summation orders: np.convolve (the oracle) and scipy's tap-by-tap lfilter, whose state is float32 too
        s64, s32, t32 = zi, zi, zi
        for k in range(pm.LFILTER_BUFFERS):
            y64, s64 = pm.ref_lfilter(b, x[k], s64)
            y32, s32 = pm.f32_lfilter(b, x[k], s32)
            u32, t32 = pm.f32_lfilter_scipy(b, x[k], t32)
            worst_y = max(worst_y, pm.worst_row(y32, y64), pm.worst_row(u32, y64))
        if ntaps > 1:
            worst_z = max(worst_z, pm.worst_row(s32, s64), pm.worst_row(t32, s64))
    print("float32 lfilter %d taps: y %.3g state %.3g" % (ntaps, worst_y, worst_z))
    assert worst_y < pm.YARDSTICK["lfilter"] and worst_z < pm.YARDSTICK["lfilter_state"]


@pytest.mark.parametrize("n", pm.HILBERT_ENGINE_SIZES + pm.HILBERT_ROCFFT_SIZES + pm.HILBERT_SMALLEST)
def test_yardstick_hilbert(n):
    worst = 0.0
    for C in pm.HILBERT_BATCHES:
        x = pm.spectral_input(C, n, n, False, 5)
        worst = max(worst, pm.worst_row(pm.f32_hilbert(x), pm.ref_hilbert(x)))
    print("float32 hilbert %d: %.3g" % (n, worst))
    assert worst < pm.YARDSTICK["hilbert"]


@pytest.mark.parametrize("n", pm.DISC_SIZES)
def test_yardstick_discriminator(n):
    worst = 0.0
    for C in pm.DISC_BATCHES:
        iq = pm.discriminator_input(C, n, 6)
        for scale in (1.0,) + pm.DISC_SCALES:
            scaled = (iq.astype(np.complex128) * scale).astype(np.complex64)
            worst = max(worst, pm.worst_row(pm.f32_discriminator(scaled), pm.ref_discriminator(scaled)))
    print("float32 discriminator %d: %.3g" % (n, worst))
    assert worst < pm.YARDSTICK["discriminator"]


@pytest.mark.parametrize("mult", pm.PLL_INTEGER + pm.PLL_PRINCIPAL)
def test_yardstick_pll_phase(mult):
    worst = 0.0
    for count in pm.PLL_COUNTS:
        z = pm.pll_input(count, mult, 7)
        for want_imag in (0, 1):
            got = pm.f32_pll(z, mult, want_imag)
            assert np.all(np.isfinite(got))
            worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - pm.ref_pll(z, mult, want_imag)))))
    print("float32 pll_phase mult %g: %.3g (bound %.3g)" % (mult, worst, pm.pll_yardstick(mult)))
    assert worst < pm.pll_yardstick(mult)


def test_what_numpy_does_outside_the_range_and_at_zero():
    """The patterns tests/test_hip_primitives.py holds the device to.  Far outside pll_magnitude_range the complex64
    power overflows (inf / inf) or underflows (0 / 0): NaN everywhere, for every mult with |mult| >= 1.  z = 0: NaN for
    every mult but 0, where numpy's power is 1 whatever the base: real 1, imaginary 0."""
    for mult in pm.PLL_INTEGER + pm.PLL_PRINCIPAL:
        zero = np.zeros(4, np.complex64)
        for want_imag in (0, 1):
            at0 = pm.f32_pll(zero, mult, want_imag)
            if mult == 0:
                assert np.all(at0 == (0.0 if want_imag else 1.0))
            else:
                assert np.all(np.isnan(at0)), (mult, at0)
            if abs(mult) >= 1:
                for outside in (1, -1):
                    got = pm.f32_pll(pm.pll_input(4099, mult, 7, outside), mult, want_imag)
                    print("mult %g outside %+d imag %d: NaN share %.3f" % (mult, outside, want_imag, np.isnan(got).mean()))
                    assert np.all(np.isnan(got)), (mult, outside)
