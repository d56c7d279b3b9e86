"""The batched single-stage entry points of include/rcfm.h ("primitives"): float64 references, seeded inputs, the
per-row error metric and the tolerances (no test functions; CPU only).

References -- radiocore_oracle's restatements of the scipy calls, evaluated on inputs cast UP to float64 / complex128
(the oracle computes in the dtype it is handed, so the up-cast is what makes it the high-precision reference):

    resample        oracle.resample with the fftshifted periodic Hamming window (decimate.py:32-48)
    filtfilt        oracle.filtfilt_fir (step by step: odd extension by 3 ntaps, lfilter_zi, forward, backward)
    lfilter         oracle.fir_filter (outputs and final state)
    hilbert         oracle.hilbert
    discriminator   angle(x[t] conj x[t-1]) / pi, d[0] = 0 (signal_edges.steps)
    pll_phase       cos / sin(mult arg z)

Inputs -- every row of a batch is drawn separately and row amplitudes are spread over three decades (row_amplitudes),
so a row read with the wrong stride or swapped with a neighbour cannot hide under the loudest row's peak: the metric
(row_errors) is max|delta_c| / max|ref_c| per row, worst row reported, no weighting, no sample left out.

Tolerances -- YARDSTICK[...] is an upper bound of the error the SAME mathematics has in float32 / complex64 on the CPU
(scipy.fft on complex64, the oracle functions fed float32) against the float64 reference, on these very inputs:
tests/test_primitives_model.py evaluates that error for every case and asserts it below the constant.  The device is
held to gpu_bound(constant) = min(4 x constant, 1e-4): the factor 4 covers another summation order (the engine's
factorisation is not pocketfft's, tiled FIR sums are not np.convolve's), and nothing is looser than conftest.TOL.
The constants are properties of float32 and of the inputs; nothing the kernels return enters them.
"""

import numpy as np

import radiocore_oracle as oracle
import signal_edges

TOL = 1e-4                      # conftest.TOL
STEP_BOUND = signal_edges.STEP_BOUND
ROW_STEP = 0.7                  # phase step / pi from the last sample of row c to the first of row c + 1
NYQUIST_SHARE = 0.05            # least share of a row's energy in its Nyquist bin(s)

# float32-on-the-CPU error bounds (see the module docstring).  Relative to the row's peak, except pll (absolute: the
# outputs lie on the unit circle), where it grows with the number of float32 complex multiplications.
# (the worst float32 figure over the cases of each entry point, as test_primitives_model.py prints it, plus a quarter)
YARDSTICK = {
    "resample_complex": 6e-7,       # scipy.fft in complex64: 4.9e-7 at the prime length, 2 .. 3e-7 elsewhere
    "resample_real": 4.5e-7,        # 3.4e-7
    "filtfilt": 3.1e-7,             # oracle.filtfilt_fir in float32: 2.5e-7
    "lfilter": 2.3e-7,              # oracle.fir_filter (np.convolve) and scipy.signal.lfilter in float32: 1.85e-7
    "lfilter_state": 3.1e-7,        # scipy.signal.lfilter's float32 final state: 2.5e-7 (the oracle forms it in float64)
    "hilbert": 6e-7,                # 4.8e-7 at the odd and the prime length, 2.8e-7 elsewhere
    "discriminator": 1.7e-7,        # numpy's complex64 product and float32 angle: 1.3e-7
}
PLL_INTEGER = (1, 2, 3, 7, 64)
PLL_PRINCIPAL = (0.5, 2.5, 65, -1, 0)


# rcfm_pll_phase, absolute, per mult: the worst error of numpy's complex64 power (the oracle's PLL.real / image on a
# complex64 baseline) against cos / sin(mult arg z) in float64 over PLL_COUNTS, plus a quarter; never below one float32
# eps, which no float32 result on the unit circle is held closer than (mult = 0: numpy's answer is exactly 1 / 0).
# It grows with mult: numpy multiplies integer exponents out (|mult| < 100), one float32 complex product per step.
PLL_YARDSTICK = {
    1: 2.05e-7, 2: 2.05e-7, 3: 2.15e-7, 7: 3.8e-7, 64: 4.2e-6,          # measured 1.63e-7 .. 3.35e-6
    0.5: 2.05e-7, 2.5: 1.0e-6, 65: 4.45e-6, -1: 2.05e-7, 0: 1.2e-7,     # measured 1.64e-7, 7.98e-7, 3.55e-6, 1.62e-7, 0
}


def pll_yardstick(mult):
    return PLL_YARDSTICK[mult]


def gpu_bound(yardstick):
    return min(4.0 * yardstick, TOL)


def pll_gpu_bound(mult):
    """4 x the float32 evaluation's bound; absolute, so conftest.TOL (a share of a peak of 1) caps it as well."""
    return min(4.0 * pll_yardstick(mult), TOL)


# ---- cases (one place: test_primitives_model.py pins on the CPU exactly what test_hip_primitives.py runs) --------------

BATCHES = (1, 2, 3, 5)
# (n, m): complex; the route (engine / rocFFT, windowed or not) is read from rcfm_fft_describe by the GPU test
RESAMPLE_COMPLEX = [(100000, 2500), (100000, 100000), (6000, 1200),                       # engine lengths, down and equal
                    (1001, 201), (1001, 200), (1000, 201), (1000, 200),                   # down, four parities
                    (201, 1001), (200, 1001), (201, 1000), (200, 1000),                   # up, four parities
                    (10007, 10007), (4099, 512), (600, 2400)]                             # prime lengths; engine lengths, up
RESAMPLE_REAL = [(1001, 201), (1001, 200), (1000, 201), (1000, 200),                      # down: nyq_factor 2 for even m
                 (201, 1001), (200, 1001), (201, 1000), (200, 1000),                      # up: nyq_factor 1/2 for even n
                 (1000, 1000), (1001, 1001), (240000, 48000), (48000, 240000)]
FILTFILT_TAPS = (2, 40, 41, 61, 101)
FILTFILT_SIZES = (1023, 1024, 1025, 2049, 5000)            # plus 3 ntaps + 1; kept where n > 3 ntaps
FILTFILT_BATCHES = (1, 3, 4)
LFILTER_TAPS = (1, 2, 51, 200)
LFILTER_BATCHES = (1, 3)
LFILTER_BUFFERS = 3


def lfilter_sizes(ntaps):
    return sorted({n for n in (1, 10, ntaps - 2, ntaps - 1, ntaps, 1024, 1025, 4800) if n >= 1})


def filtfilt_sizes(ntaps):
    return sorted({n for n in (3 * ntaps + 1,) + FILTFILT_SIZES if n > 3 * ntaps})


HILBERT_BATCHES = (1, 2, 5)
HILBERT_ENGINE_SIZES = (6000, 44100, 240000)
HILBERT_ROCFFT_SIZES = (44103, 10007, 1002)                # odd (3 * 61 * 241), prime, even (2 * 3 * 167): no engine plan
HILBERT_SMALLEST = (256, 16)                               # the smallest n >= 16 of the engine / of rocFFT (the GPU test checks)
PLL_COUNTS = (1, 255, 256, 257, 10 ** 6 + 3)
DISC_BATCHES = (1, 3)
DISC_SIZES = (1, 2, 255, 256, 257, 100003)
DISC_SCALES = (1e-6, 1e3)


# ---- metric -------------------------------------------------------------------------------------------------------------

def row_errors(got, ref):
    """max|got_c - ref_c| / max|ref_c| per row of [C][...] arrays (a row of zeros is measured against 1)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    peak = np.max(np.abs(ref), axis=1)
    peak = np.where(peak > 0, peak, 1.0)
    return np.max(np.abs(got.astype(ref.dtype) - ref), axis=1) / peak


def worst_row(got, ref):
    return float(np.max(row_errors(got, ref)))


def segment_errors(got, ref, edge):
    """(head, interior, tail): worst row of max|delta| over the first `edge` samples, what lies between and the last
    `edge`, each relative to the WHOLE row's peak."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    peak = np.max(np.abs(ref), axis=1)
    peak = np.where(peak > 0, peak, 1.0)
    d = np.abs(got - ref) / peak[:, None]
    n = d.shape[1]
    inner = d[:, edge:n - edge]
    return float(d[:, :edge].max()), float(inner.max()) if inner.size else 0.0, float(d[:, n - edge:].max())


# ---- inputs ---------------------------------------------------------------------------------------------------------------

def row_amplitudes(C):
    """1 down to 1e-3, evenly in the logarithm (one row: 1)."""
    return np.logspace(0.0, -3.0, C) if C > 1 else np.ones(1)


def _rng(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


def nyquist_bins(n, m=None):
    """The bins of the length-n spectrum that the Nyquist rules of scipy.signal.resample / hilbert single out for an
    output of m samples: +-K, K = min(n, m) // 2 (as indices into the n-point FFT)."""
    K = min(n, n if m is None else m) // 2
    return sorted({K % n, (n - K) % n})


def spectral_input(C, n, m, cplx, seed):
    """[C][n] float32 / complex64: per row, unit white noise (per component) plus
        a DC level of 0.5 (complex: 0.5 - 0.3j),
        a tone exactly in the Nyquist bin K = min(n, m) // 2 -- complex: 0.6 in +K and 0.45 in -K with drawn phases, so
        that NYQ_DOWN's merge of the two and NYQ_UP's halving and mirror all act on signal; real: 0.6 cos --,
        tones of 0.4 in the bins K - 1 and K + 1 (the latter where it exists below n / 2),
    all times the row's amplitude.  A tone of amplitude a puts a n into its bin, against sqrt(n) from the noise."""
    t = np.arange(n, dtype=np.float64)
    K = min(n, m) // 2
    rows = []
    for c, amp in enumerate(row_amplitudes(C)):
        r = _rng(seed, n, m, c, cplx)
        ph = r.uniform(0, 2 * np.pi, 6)
        if cplx:
            x = r.standard_normal(n) + 1j * r.standard_normal(n) + (0.5 - 0.3j)
            x = x + 0.6 * np.exp(1j * (2 * np.pi * K * t / n + ph[0]))
            if 2 * K != n:          # (at K = n / 2 the two are one bin and could cancel)
                x = x + 0.45 * np.exp(-1j * (2 * np.pi * K * t / n + ph[1]))
            for j, k in enumerate((K - 1, K + 1)):
                if 0 < k < n / 2:
                    x = x + 0.4 * np.exp(1j * (2 * np.pi * k * t / n + ph[2 + j])) \
                        + 0.4 * np.exp(-1j * (2 * np.pi * k * t / n + ph[4 + j]))
        else:
            x = r.standard_normal(n) + 0.5
            # (at K = n / 2 the cosine is +-cos(phase): keep the phase away from pi / 2)
            x = x + 0.6 * np.cos(2 * np.pi * K * t / n + (0.3 if 2 * K == n else ph[0]))
            for j, k in enumerate((K - 1, K + 1)):
                if 0 < k < n / 2:
                    x = x + 0.4 * np.cos(2 * np.pi * k * t / n + ph[2 + j])
        rows.append(amp * x)
    return np.array(rows).astype(np.complex64 if cplx else np.float32)


def nyquist_share(x, m=None):
    """Per row: energy in nyquist_bins / total energy."""
    X = np.abs(np.fft.fft(np.asarray(x).astype(np.complex128), axis=1)) ** 2
    return X[:, nyquist_bins(x.shape[1], m)].sum(axis=1) / X.sum(axis=1)


def noise_rows(C, n, seed):
    """[C][n] float32 white noise, row amplitudes spread."""
    return np.array([a * _rng(seed, n, c).standard_normal(n) for c, a in enumerate(row_amplitudes(C))]).astype(np.float32)


def ramp_rows(C, n):
    """[C][n] float32: a_c + b_c t, a different offset and slope (of either sign) per row, row amplitudes spread."""
    t = np.arange(n, dtype=np.float64) / n
    off, slope = (0.3, -0.5, 1.0, 0.1, -0.8), (1.0, 0.7, -1.2, 2.0, -0.4)
    return np.array([a * (off[c % 5] + slope[c % 5] * t) for c, a in enumerate(row_amplitudes(C))]).astype(np.float32)


def filtfilt_input(C, n, seed):
    """noise_rows on top of ramp_rows: ends that are far from zero, so the odd extension matters."""
    return (noise_rows(C, n, seed).astype(np.float64) + ramp_rows(C, n)).astype(np.float32)


def filter_taps(kind, ntaps, seed=0):
    """float32 taps with unit DC gain.  "firwin": a Hamming low-pass at 0.2 of Nyquist (symmetric);
    "random": drawn, NOT symmetric: positive taps under a decaying envelope, so that sum|b| = sum b = 1 and the float32
    rounding of the taps moves the DC gain by no more than a few 1e-8 (a ramp then comes back as it went in)."""
    if kind == "firwin":
        m = np.arange(ntaps) - 0.5 * (ntaps - 1)
        h = 0.2 * np.sinc(0.2 * m)
        if ntaps > 1:
            h = h * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(ntaps) / (ntaps - 1)))
    else:
        r = _rng(seed, ntaps, 77)
        h = r.uniform(0.2, 1.0, ntaps) * np.exp(-np.arange(ntaps) / max(1.0, ntaps / 3.0))
    h = (h / np.sum(h)).astype(np.float32)
    return h


def lfilter_input(C, n, ntaps, buffers, seed):
    """(x [buffers][C][n], zi [C][ntaps - 1]) float32: a different initial state per row, at the row's amplitude."""
    x = np.array([noise_rows(C, n, seed + 1000 * b) for b in range(buffers)])
    zi = noise_rows(C, max(ntaps - 1, 1), seed + 7)[:, :ntaps - 1]
    return x, np.ascontiguousarray(zi)


def discriminator_input(C, n, seed):
    """[C][n] complex64: phase steps drawn uniformly within +-STEP_BOUND pi, magnitudes within [0.5, 1.5) of the row's
    amplitude.  Row c + 1 BEGINS ROW_STEP pi beyond the phase row c ENDS at: a difference taken across the row boundary
    would put ROW_STEP, not 0, into d[c + 1][0]."""
    rows, phase0 = [], 0.4
    for c, amp in enumerate(row_amplitudes(C)):
        r = _rng(seed, n, c, 5)
        step = r.uniform(-STEP_BOUND, STEP_BOUND, n)
        step[0] = 0.0
        phase = phase0 + np.pi * np.cumsum(step)
        rows.append(amp * r.uniform(0.5, 1.5, n) * np.exp(1j * phase))
        phase0 = phase[-1] + ROW_STEP * np.pi
    return np.array(rows).astype(np.complex64)


def pll_magnitude_range(mult):
    """(lo, hi): the |z| for which |z|^mult is a normal float32 with room for the smaller component of z^mult:
    2^-100 <= |z|^|mult| <= 2^100 (float32 holds 2^-126 .. 2^127), i.e. |z| within 2^(+-100 / |mult|); for |mult| < 1
    (0 included) |z| itself within 2^+-100.  The multiply-out branch of the kernel forms z^k, k <= mult, and needs this; its
    principal branch uses arg z alone and does not, but the complex64 evaluation it is measured by (numpy's power) does."""
    p = max(1.0, abs(float(mult)))
    return 2.0 ** (-100.0 / p), 2.0 ** (100.0 / p)


def pll_input(count, mult, seed, outside=0):
    """[count] complex64: phases uniform, magnitudes log-uniform over pll_magnitude_range(mult).  outside = +1 / -1:
    magnitudes whose mult-th power lies between 2^200 and 2^300 (2^-300 and 2^-200): far beyond float32 either way."""
    r = _rng(seed, count, int(mult * 2), outside + 1)
    lo, hi = pll_magnitude_range(mult)
    e = r.uniform(np.log2(lo), np.log2(hi), count)
    if outside:
        e = outside * r.uniform(200.0, 300.0, count) / max(1.0, abs(float(mult)))
    z = np.exp2(e) * np.exp(1j * r.uniform(-np.pi, np.pi, count))
    return z.astype(np.complex64)


# ---- float64 references -----------------------------------------------------------------------------------------------------

def _up(x):
    x = np.asarray(x)
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def ref_resample(x, m):
    x = _up(x)
    w = oracle.shifted_window("hamm", x.shape[1])
    return np.array([oracle.resample(row, m, window=w) for row in x])


def ref_filtfilt(b, x):
    return np.array([oracle.filtfilt_fir(_up(b), row) for row in _up(x)])


def ref_lfilter(b, x, zi):
    """x [C][n], zi [C][ntaps - 1] -> (y [C][n], zf [C][ntaps - 1])."""
    out = [oracle.fir_filter(_up(b), row, z) for row, z in zip(_up(x), _up(zi))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(len(out), -1)


def ref_hilbert(x):
    return np.array([oracle.hilbert(row) for row in _up(x)])


def ref_discriminator(iq):
    return np.array([signal_edges.steps(row) for row in iq])


def ref_pll(z, mult, want_imag):
    th = float(mult) * np.angle(_up(z))
    return np.sin(th) if want_imag else np.cos(th)


# ---- the same mathematics in float32 / complex64 on the CPU (the yardstick) ---------------------------------------------------

def f32_resample(x, m):
    import scipy.fft
    x = np.asarray(x)
    n = x.shape[1]
    real = np.isrealobj(x)
    w = oracle.shifted_window("hamm", n).astype(np.float32)
    out = []
    for row in x:
        X = scipy.fft.rfft(row) if real else scipy.fft.fft(row)
        assert X.dtype == np.complex64
        Y = oracle.resample_spectrum(X, m, n, real, w)
        y = scipy.fft.irfft(Y, m) if real else scipy.fft.ifft(Y)
        out.append(y * np.float32(float(m) / float(n)))
    out = np.array(out)
    assert out.dtype == (np.float32 if real else np.complex64)
    return out


def f32_filtfilt(b, x):
    out = np.array([oracle.filtfilt_fir(np.asarray(b, np.float32), row) for row in np.asarray(x, np.float32)])
    assert out.dtype == np.float32
    return out


def f32_lfilter_scipy(b, x, zi):
    """scipy.signal.lfilter in float32: the transposed direct form, one tap after the other -- a second float32 summation
    order next to f32_lfilter's np.convolve, and the only one whose final state is formed in float32."""
    import scipy.signal
    b = np.asarray(b, np.float32)
    x, zi = np.asarray(x, np.float32), np.asarray(zi, np.float32)
    if len(b) == 1:
        return scipy.signal.lfilter(b, np.ones(1, np.float32), x, axis=1), zi
    y, zf = scipy.signal.lfilter(b, np.ones(1, np.float32), x, axis=1, zi=zi)
    assert y.dtype == np.float32 and zf.dtype == np.float32
    return y, zf


def f32_lfilter(b, x, zi):
    b = np.asarray(b, np.float32)
    out = [oracle.fir_filter(b, row, z) for row, z in zip(np.asarray(x, np.float32), np.asarray(zi, np.float32))]
    y, zf = np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(len(out), -1)
    assert y.dtype == np.float32 and zf.dtype == np.float32
    return y, zf


def f32_hilbert(x):
    import scipy.fft
    out = []
    for row in np.asarray(x, np.float32):
        n = len(row)
        X = scipy.fft.fft(row)
        assert X.dtype == np.complex64
        h = np.zeros(n, np.float32)
        h[0] = 1
        h[1:(n + 1) // 2] = 2
        if n % 2 == 0:
            h[n // 2] = 1
        out.append(scipy.fft.ifft(X * h))
    return np.array(out)


def f32_discriminator(iq):
    iq = np.asarray(iq, np.complex64)
    d = np.zeros(iq.shape, np.float32)
    d[:, 1:] = np.angle(iq[:, 1:] * np.conj(iq[:, :-1])) / np.float32(np.pi)
    return d


def f32_pll(z, mult, want_imag):
    """The oracle's PLL.real / PLL.image on a complex64 baseline: numpy's complex64 power."""
    p = oracle.PLL()
    p._baseline = np.asarray(z, np.complex64)
    with np.errstate(all="ignore"):
        return p.image(mult) if want_imag else p.real(mult)
