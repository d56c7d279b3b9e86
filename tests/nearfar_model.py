"""Near-far test model (no test functions): weak AM / SSB channels next to strong ones.

On the FFT-engine routes AM and SSB carry two channels in one complex transform: AM packs the envelope rows
2P and 2P + 1 as the real and imaginary part of one B-point transform and unpacks them by symmetry, SSB packs the two
Hermitian audio spectra Y0 + j Y1 into one inverse transform and reads Re / Im.  A float32 transform rounds at the scale
of its largest member, so without care a weak channel is rounded at the scale of its partner.  The reference
demodulates every channel by itself.

    levels      exact powers of two, 2^-k for k in LEVELS_K: 0, 42, 60 and 78 dB below the strong rows
    rows        am_model.station / ssb_model.station at level 1 (each with noise relative to its own level, so no
                sideband is empty), row i times pattern(k)[i]
    pattern     [1, 2^-k, 2^-k, 1, 2^-k]: pairs (strong, weak) and (weak, strong), and a lone weak last row
    expected    AM and SSB are scale-free and 2^-k is exact in float32: the expected audio of a scaled row is that of
                the level-1 row, evaluated in float64 (expect64); expect32 is the oracle's own float32 evaluation
    paired_float32   numpy's complex64 transforms standing in for the device's pair routes
    from_spectrum    float64 audio of one Tuner channel from a wideband spectrum given as complex128
"""

import numpy as np

import am_model
import radiocore_oracle as oracle
import ssb_model

LEVELS_K = (0, 7, 10, 13)
BATCH = 5
WEAK = (1, 2, 4)          # rows of pattern(k) at 2^-k; 1 sits in the imaginary slot of its pair, 2 in the real slot
STRONG = (0, 3)
LONE = 4                  # the last row of an odd batch has no partner

# (kind, B, A) of the demodulator-level cases: the smallest shapes at which each route exists (tests/test_hip_am.py
# ROUTES, tests/test_hip_ssb.py STANDALONE)
AM_ENGINE = ("AM", 25000, 8000)
AM_ROCFFT = ("AM", 22000, 8000)
SSB_ENGINE = (12500, 8000)
SSB_ROCFFT = (3001, 1001)
GEOMETRIES = [AM_ENGINE, AM_ROCFFT, ("USB",) + SSB_ENGINE, ("LSB",) + SSB_ENGINE, ("USB",) + SSB_ROCFFT]
SEED = 4


def pattern(k):
    w = 2.0 ** -int(k)
    return np.array([1.0, w, w, 1.0, w])


def station_indices(kind, A, seed=SEED, count=BATCH):
    """The first `count` stations whose compared sideband keeps a tone inside the audio band, below 0.45 A Hz.  At
    A = 8000 that is stations 0 .. count - 1 (ssb_model's tones end at 2700 Hz, am_model's at 3400 Hz); at A = 1001 the
    decimation drops everything above 500 Hz, and a station without a tone below that is an empty sideband, which the
    RMS division makes ill conditioned for any float32 evaluation (tests/test_hip_ssb.py's docstring)."""
    if kind == "AM":
        return list(range(count))
    out, i = [], 0
    while len(out) < count:
        tones = ssb_model.station_tones(i, seed)[1 if kind == "LSB" else 0]
        if min(f for f, _, _ in tones) < 0.45 * A:
            out.append(i)
        i += 1
    return out


def unit_rows(kind, B, A, seed=SEED, count=BATCH):
    """complex64 [count, B]: the stations of station_indices at level 1."""
    mk = am_model.station if kind == "AM" else ssb_model.station
    return np.stack([mk(i, B, seed, level=1.0) for i in station_indices(kind, A, seed, count)]).astype(np.complex64)


def scaled(rows, k):
    """rows times pattern(k), complex64: every factor is a power of two, so the product is exact."""
    return (rows * pattern(k)[:len(rows), None].astype(np.float32)).astype(np.complex64)


def _tail(kind, v):
    if kind != "AM":
        return ssb_model.normalise(v)
    c = float(np.mean(v))
    if not c > 0:
        return np.zeros((len(v), 1))
    return np.clip(v / c - 1.0, -0.999, 0.999)[:, None]


def signal64(kind, iq, B, A):
    """v in float64: what the tail of the demodulator sees (AM: the decimated envelope of the complex64 samples, the
    envelope itself rounded to float32 as include/rcfm.h defines it; USB / LSB: the decimated sideband)."""
    x = np.asarray(iq).astype(np.complex64)
    if kind == "AM":
        e = np.abs(x).astype(np.float32).astype(np.float64)
        return np.asarray(oracle.Decimate(B, A).run(e), np.float64)
    return ssb_model.sideband(oracle, x, B, A, kind == "LSB")


def expect64(kind, iq, B, A):
    """Expected audio of one channel's samples, float64 [A, 1], every transform in float64."""
    out = _tail(kind, signal64(kind, iq, B, A))
    assert out.dtype == np.float64
    return out


def signal32(kind, iq, B, A):
    """signal64 as the oracle itself evaluates it on float32 input: numpy keeps single precision through its
    transforms, so Decimate on a float32 envelope and the sideband mask on complex64 samples are float32 end to end."""
    x = np.asarray(iq).astype(np.complex64)
    if kind == "AM":
        v = oracle.Decimate(B, A).run(np.abs(x).astype(np.float32))
    else:
        H = ssb_model.mask(B, kind == "LSB").astype(np.float32)
        s = np.real(np.fft.ifft(H * np.fft.fft(x)))
        assert s.dtype == np.float32
        v = oracle.Decimate(B, A).run(s)
    assert v.dtype == np.float32
    return v


def expect32(kind, iq, B, A):
    """The oracle's own float32 evaluation of one row by itself."""
    return _tail(kind, np.asarray(signal32(kind, iq, B, A), np.float64))


# ---- with the stateful AGC (tests/agc_model.py) ------------------------------------------------------------------------

AGC_K = 13
AGC_BUFFERS = 2


def agc_case(kind, B, A):
    """Two consecutive buffers of pattern(AGC_K): (units [buf] complex64 [5, B] at level 1, v [buf][row] float64 at
    level 1, (decay_samples, level, floor)).  The floor is agc_model.chain_floor of the WEAK level, 0.1 of the largest
    weak row's peak, so that the weak rows are followed and not floored."""
    import agc_model
    units = [unit_rows(kind, B, A, SEED + buf) for buf in range(AGC_BUFFERS)]
    vs = [[signal64(kind, x, B, A) for x in u] for u in units]
    floor = agc_model.chain_floor([v * 2.0 ** -AGC_K for buf in vs for v in buf])
    return units, vs, agc_model.chain_settings(kind, A, floor)


# ---- the pair routes in numpy ------------------------------------------------------------------------------------------

def _real_dtype(ctype):
    return np.float32 if ctype == np.complex64 else np.float64


def _decimate_half(S, B, A, ctype):
    """Decimate's spectrum side on the half spectrum S [B // 2 + 1] of a real signal -> Y [A // 2 + 1], in ctype."""
    W = oracle.shifted_window("hamm", B).astype(_real_dtype(ctype))
    Y = oracle.resample_spectrum(S.astype(ctype, copy=True), A, B, True, W)
    assert Y.dtype == ctype
    return Y


def _am_pair(x0, x1, B, A, ctype):
    """Two envelopes as the real and imaginary part of one B-point transform, unpacked by symmetry for the decimation
    and packed again for the inverse transform (run_pair_decim, csrc/demod.hip)."""
    rt = _real_dtype(ctype)
    e0 = np.abs(x0).astype(np.float32).astype(rt)
    e1 = (np.abs(x1).astype(np.float32).astype(rt)) if x1 is not None else np.zeros(B, rt)
    Z = np.fft.fft((e0 + 1j * e1).astype(ctype))
    assert Z.dtype == ctype
    k = np.arange(B // 2 + 1)
    Zm = np.conj(Z[(B - k) % B])
    halves = [(0.5 * (Z[k] + Zm)).astype(ctype), (-0.5j * (Z[k] - Zm)).astype(ctype)]
    if x1 is None:
        halves = halves[:1]
    # the decimating tile keeps the pair together through the inverse transform: V0 + j V1, audio in Re / Im
    V = [_hermitian(_decimate_half(S, B, A, ctype), A) for S in halves]
    z = np.fft.ifft(V[0] if x1 is None else (V[0] + 1j * V[1]).astype(ctype)) * rt(A / B)
    assert z.dtype == ctype
    return [z.real] if x1 is None else [z.real, z.imag]


def _hermitian(Y, A):
    """Full A-point spectrum of the real signal whose half spectrum is Y [A // 2 + 1]."""
    H = np.zeros(A, Y.dtype)
    H[:A // 2 + 1] = Y
    j = np.arange(1, (A + 1) // 2)
    H[A - j] = np.conj(Y[j])
    if A % 2 == 0:
        H[A // 2] = Y[A // 2].real
    H[0] = Y[0].real
    return H


def _ssb_pair(x0, x1, B, A, lower, ctype):
    """Each row's own B-point transform (the device's pruned FFT_B runs row by row), the sideband's half spectrum,
    Decimate's weights, then Y0 + j Y1 through ONE inverse A-point transform."""
    rt = _real_dtype(ctype)
    k = np.arange(B // 2 + 1)

    def half(x):
        X = np.fft.fft(x.astype(ctype))
        S = np.conj(X[(B - k) % B]) if lower else X[k].copy()
        S[0] = 0.0
        if B % 2 == 0:
            S[B // 2] = 0.0
        return _hermitian(_decimate_half(S.astype(ctype), B, A, ctype), A)

    Z = half(x0)
    if x1 is not None:
        Z = (Z + 1j * half(x1)).astype(ctype)
    z = np.fft.ifft(Z) * rt(A / B)
    assert z.dtype == ctype
    return [z.real] if x1 is None else [z.real, z.imag]


def paired(kind, rows, B, A, ctype=np.complex64):
    """Audio [len(rows), A, 1] (float64 after the tail) of the rows taken two by two through shared transforms in
    `ctype`; an odd last row travels alone.  complex128 gives expect64 (tests/test_nearfar_model.py checks that)."""
    rows = np.asarray(rows).astype(np.complex64)
    out = []
    for p in range(0, len(rows), 2):
        x0, x1 = rows[p], (rows[p + 1] if p + 1 < len(rows) else None)
        vs = _am_pair(x0, x1, B, A, ctype) if kind == "AM" else _ssb_pair(x0, x1, B, A, kind == "LSB", ctype)
        out += [_tail(kind, np.asarray(v, np.float64)) for v in vs]
    return np.stack(out)


def paired_float32(kind, rows, B, A):
    """The float32 emulation of the pair route: pack, complex64 transform, unpack, decimate, tail."""
    return paired(kind, rows, B, A, np.complex64)


# ---- truth from a wideband spectrum ------------------------------------------------------------------------------------

def from_spectrum(oracle, X, n, roll, B, A, kind):
    """float64 audio [A, 1] of the channel (roll, B) of the wideband spectrum X (complex128 [n], as the device or the
    oracle holds it after load): radiocore_oracle.tuner_channel_spectrum and the inverse transform in float64, then AM's
    expectation on those samples, or ssb_model.direct for USB / LSB."""
    X = np.asarray(X)
    assert X.dtype == np.complex128 and len(X) == n
    if kind == "AM":
        iq = np.fft.ifft(oracle.tuner_channel_spectrum(X, n, roll, B)) * (float(B) / float(n))
        e = np.abs(iq).astype(np.float32).astype(np.float64)       # the envelope is a float32 quantity (include/rcfm.h)
        out = _tail("AM", np.asarray(oracle.Decimate(B, A).run(e), np.float64))
    else:
        out = ssb_model.normalise(ssb_model.direct(oracle, X, roll, B, A, kind == "LSB"))
    assert out.dtype == np.float64
    return out
