"""rcfm_tuner_run, the stage every channel passes through: float64 reference, seeded inputs, the per-channel error
metric, the case table, a restatement of which form the library picks, and the tolerances (no test functions; CPU only).

Reference -- ref_channel(X, n, roll, B): oracle.tuner_channel_spectrum on X cast UP to complex128, np.fft.ifft, x B / n:
tuner.py:151-161 (np.roll + scipy.signal.resample(domain="freq") with the fftshifted Hann window).  np.roll is circular,
so it is exact for any roll, band edges included.

A second float64 statement -- channel_spectrum(X, n, roll, B): the way the kernels read it.  Output bin k of a channel
comes from wideband bin (base + d) mod n, base = (n - roll) mod n, d = k on the positive side (k <= B // 2) and k - B on
the negative one, weighted with
    w(d) = a0 + (1 - a0) cos(2 pi d / n + delta),    a0 = 1/2,  delta = pi / n for odd n, else 0;
for even B < n (B > 2) bin B // 2 also receives X[base - B // 2] w(-B // 2) (NYQ_DOWN, the merge).  Its `defect` argument
builds the deliberately broken copies that tests/test_tuner_model.py shows the inputs can see.

Forms -- gather_form() restates rcfm_tuner_s::run and rcfm_tuner_s::fast_gather_ok (radio-core_amd/csrc/tuner.hip,
fused_passes.hip) from what the library reports (halo: rcfm_tuner_spectrum_layout; engines: rcfm_fft_describe):
    "tables"    no engine plan for B: k_spectrum_c2c with window tables in front of rocFFT
    "fast"      LoadTunerGatherFast: haloed spectrum (halo >= B // 2 + 1), 32-bit bases, window argument
                2 pi (B // 2 + 2) / n < 0.25 (four-term cosine series)
    "general"   LoadTunerGatherT<int32_t>: modulo indexing, cosf
The haloed spectrum [halo | n bins | halo] repeats the far ends: X[-halo:0] == X[n - halo:n], X[n:n + halo] == X[0:halo];
halo <= n / 2 (tuner_halo), else a handle keeps none.

Input -- one seeded complex noise buffer per n: every bin carries weight, so an edge bin or a merge bin cannot hide.
Metric -- per channel max|delta| / max|ref|, worst channel reported, no sample left out (primitives_model.row_errors).

Tolerances -- YARDSTICK["tuner_run"] bounds the error of the SAME arithmetic in float32 on the CPU (f32_channel: window in
float32, complex64 product, scipy.fft.ifft on complex64, float32 scale) against ref_channel over every case and roll of the
table; YARDSTICK_FFT bounds scipy.fft.fft on complex64 against float64 on the inputs, relative to the spectrum's peak.
tests/test_tuner_model.py evaluates both and asserts them below the constants.  The device is held to
primitives_model.gpu_bound(constant): 4 x for another summation order, never above conftest.TOL.  Nothing the kernels
return enters the constants.
"""

import functools

import numpy as np

import primitives_model as pm
import radiocore_oracle as oracle

A0 = 0.5                        # Hann
SERIES_LIMIT = 0.25             # rad: the fast form's four-term series is used below it (fused_passes.hip)

# (the worst float32 figure over the table, as test_tuner_model.py prints it, plus a quarter)
YARDSTICK = {
    "tuner_run": 3.6e-7,        # 2.86e-7 at (10125, 668); 1.65e-7 .. 2.5e-7 elsewhere; B = 1, 2: 8.9e-8
}
YARDSTICK_FFT = 3.4e-7          # scipy.fft in complex64: 2.67e-7 at the prime length, 1.7e-7 .. 2.0e-7 elsewhere

# ---- cases (one place: test_tuner_model.py pins on the CPU exactly what test_hip_tuner_gather.py runs) --------------------
# One tuner handle per row: (n, bandwidths).  A handle's halo follows its widest channel, so the bandwidths that are to
# keep a fast form share a handle with nothing wider than the general-form cases, and B == n has handles of its own.
TUNERS = (
    # n odd (3^4 5^3, engine): the window's delta != 0
    (10125, (675,        # odd, fast, 6.7 % of n
             600,        # even, fast, NYQ_DOWN
             800,        # the last B on the series side: 2 pi (B / 2 + 2) / n = 0.2495
             810,        # the first on the cosf side
             2025,       # general, odd
             2250,       # general, NYQ_DOWN
             667,        # 23 x 29: tables, odd
             668)),      # 4 x 167: tables, NYQ_DOWN
    (10125, (1,)),
    (10125, (2,)),       # even, but scipy's merge slice is empty
    (10125, (10125,)),   # B == n, odd
    # n even (engine)
    (10240, (640,        # fast, NYQ_DOWN
             625,        # fast, odd
             2560)),     # general, NYQ_DOWN
    (10240, (10240,      # B == n: even but no merge; beside a narrow channel: the halo of the widest would exceed n / 2
             640)),
    # n prime: rocFFT forward, halos by copies
    (10007, (600, 675)),
    # many tiles; a three-pass inverse
    (1_200_000, (24000, 60000, 375000)),
)
HALO_EDGE = (10240, (10236,))   # halo == n / 2 exactly: the widest handle that keeps its halos (halo test only)
SMALL_N = 20000                 # below it the literal O(n)-per-channel oracle.Tuner.run is affordable


def rolls(n, B):
    """The channels of one rcfm_tuner_run range of bandwidth B: an odd count, so the last pair has a lone member."""
    return (0,
            3,                          # base n - 3: reads the right halo
            n - 5,                      # base 5: reads the left halo
            n // 2, n // 2 + 1,         # centred on the band edge: the bins wrap through +-n / 2
            (n - B // 2) % n,           # the channel's own lower edge on bin 0 ...
            (B // 2 + 1) % n,           # ... and its upper edge just below it
            n // 3 + 1, n - n // 7)     # interior


def cases():
    """(n, B) of every (tuner, bandwidth) of the table, in order (one pair may appear in two tuners)."""
    return [(n, B) for n, bws in TUNERS for B in bws]


# ---- which form the library picks -------------------------------------------------------------------------------------------

def tuner_halo(n, bandwidths):
    """rcfm_tuner_create: whole 128-byte lines, wide enough for the widest channel (B // 2 + 2 bins); kept only while it
    fits 32-bit bases and halo <= n / 2, so that no bin belongs to both halos."""
    h = max(B // 2 + 2 for B in bandwidths)
    h = (h + 15) // 16 * 16
    return h if 2 * h <= n and n + h < 2 ** 31 else 0


def nyquist_mode(n, B):
    """"down": even B < n, B > 2 -- Y[+B/2] += X[-B/2] (for B == 2 scipy's slice is empty); else "none" (B <= n)."""
    assert B <= n
    return "down" if B % 2 == 0 and B < n and B > 2 else "none"


def series_argument(n, B):
    return 2.0 * np.pi * (B // 2 + 2) / n


def gather_form(n, halo, B, engine_for_B, engine_for_n):
    """"fast", "general" or "tables" (module docstring).  engine_for_n does not enter: rcfm_tuner_s::run never asks how
    the spectrum was produced -- it is taken so that a caller states everything the library reported."""
    assert B <= n < 2 ** 30, "the int64 general form is out of reach here"
    del engine_for_n
    if not engine_for_B:
        return "tables"
    if halo > 0 and halo >= B // 2 + 1 and series_argument(n, B) < SERIES_LIMIT:
        return "fast"
    return "general"


# ---- inputs and metric ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def noise(n):
    """[n] complex64, unit variance per component, seeded by n; read-only (shared between tests)."""
    r = np.random.default_rng([n, 20240])
    x = (r.standard_normal(n) + 1j * r.standard_normal(n)).astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def spectrum64(n):
    """np.fft.fft of noise(n) in float64; read-only."""
    X = np.fft.fft(noise(n).astype(np.complex128))
    X.setflags(write=False)
    return X


channel_errors = pm.row_errors
worst_channel = pm.worst_row


# ---- float64 reference ------------------------------------------------------------------------------------------------------

def ref_channel(X, n, roll, B):
    X = np.asarray(X).astype(np.complex128)
    assert X.shape == (n,)
    return np.fft.ifft(oracle.tuner_channel_spectrum(X, n, int(roll), int(B))) * (float(B) / float(n))


def ref_channels(X, n, B):
    """[len(rolls)][B]: every roll of the table."""
    X = np.asarray(X).astype(np.complex128)
    return np.array([ref_channel(X, n, r, B) for r in rolls(n, B)])


@functools.lru_cache(maxsize=None)
def ref_channels_of_input(n, B):
    """ref_channels from the float64 spectrum of noise(n): forward FFT + gather + inverse; read-only."""
    y = ref_channels(spectrum64(n), n, B)
    y.setflags(write=False)
    return y


# ---- the kernels' reading of it (float64; float32 below) --------------------------------------------------------------------

def signed_offsets(B):
    k = np.arange(B)
    return np.where(k <= B // 2, k, k - B)


def window(d, n, dtype=np.float64, delta=True, series=False, c1_factor=1.0, c2_factor=1.0):
    """w(d) of the module docstring in `dtype` arithmetic.  series: the fast form's c0 + t c1 + t^2 c2 + t^3 c3, t = th^2."""
    f = np.dtype(dtype).type
    th = np.asarray(d).astype(dtype) * f(2.0 * np.pi / n) + f(np.pi / n if (n % 2 and delta) else 0.0)
    a1 = 1.0 - A0
    if series:
        t = th * th
        c0, c1, c2, c3 = f(A0 + a1), f(c1_factor * -a1 / 2.0), f(c2_factor * a1 / 24.0), f(-a1 / 720.0)
        return ((t * c3 + c2) * t + c1) * t + c0
    return f(A0) + f(a1) * np.cos(th)


# What a subtly wrong kernel would compute.  The series defects act only where the series is used (SERIES_LIMIT).
SERIES_DEFECTS = {"series c1 off by 10 %": dict(c1_factor=1.1), "series c2 off by 10 %": dict(c2_factor=1.1),
                  "series c2 missing": dict(c2_factor=0.0)}
DEFECTS = ("no delta", "no merge", "negative side late", "right halo zero") + tuple(SERIES_DEFECTS)


def channel_spectrum(X, n, roll, B, defect=None, wdtype=np.float64):
    """The length-B spectrum Y of a channel (the channel is ifft(Y) B / n) in X's dtype, window in wdtype arithmetic.
    defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    X = np.asarray(X)
    base = (n - int(roll)) % n
    d = signed_offsets(B)
    if defect == "negative side late":          # bin B // 2 + 1 still read as a positive offset
        d = np.where(np.arange(B) <= B // 2 + 1, np.arange(B), d)
    kw = dict(dtype=wdtype, delta=defect != "no delta")
    if defect in SERIES_DEFECTS:
        kw.update(series=series_argument(n, B) < SERIES_LIMIT, **SERIES_DEFECTS[defect])

    def fetch(dd):
        v = X[(base + dd) % n]
        if defect == "right halo zero":         # elements behind bin n - 1 of a haloed spectrum
            v = np.where(base + dd >= n, 0, v)
        return v

    Y = (fetch(d) * window(d, n, **kw)).astype(X.dtype)
    if nyquist_mode(n, B) == "down" and defect != "no merge":
        h = np.array([-(B // 2)])
        Y[B // 2] += (fetch(h) * window(h, n, **kw)).astype(X.dtype)[0]
    return Y


def model_channel(X, n, roll, B, defect=None):
    X = np.asarray(X).astype(np.complex128)
    return np.fft.ifft(channel_spectrum(X, n, roll, B, defect)) * (float(B) / float(n))


def f32_channel(X, n, roll, B):
    """The yardstick: window in float32, complex64 product, scipy.fft.ifft on complex64, float32 scale."""
    import scipy.fft
    X = np.asarray(X)
    assert X.dtype == np.complex64
    Y = channel_spectrum(X, n, roll, B, wdtype=np.float32)
    assert Y.dtype == np.complex64
    y = scipy.fft.ifft(Y) * np.float32(float(B) / float(n))
    assert y.dtype == np.complex64
    return y


def f32_spectrum(n):
    """scipy.fft.fft of noise(n) in complex64 (YARDSTICK_FFT, and the spectrum f32_channel is fed on the CPU)."""
    import scipy.fft
    X = scipy.fft.fft(noise(n))
    assert X.dtype == np.complex64
    return X


def literal_channel(X, n, roll, B):
    """oracle.Tuner.run: np.roll of the whole spectrum and the full-length window, O(n)."""
    t = oracle.Tuner()
    t._buffer = np.asarray(X).astype(np.complex128)
    t._input_frequency, t._input_bandwidth = 0.0, float(n)
    t._bounds = [oracle.Channel(0, B, None, -float(roll))]
    return t.run(0)
