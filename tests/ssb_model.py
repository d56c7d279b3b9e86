"""SSB test model (no test functions): seeded two-sideband signals and the expected audio of the USB / LSB demodulators.

The expectation follows include/rcfm.h (RCFM_USB / RCFM_LSB) from the oracle's own pieces, in float64 on the complex64
samples:
    X = fft(x);  H_usb[k] = 2 for 1 <= k <= (B-1)//2, else 0;  H_lsb[k] = H_usb[(B - k) mod B];  s = Re(ifft(H X));
    v = radiocore_oracle.Decimate(B, A).run(s);  g = sqrt(mean(v**2));
    audio = clip(LEVEL * v / g, -0.999, 0.999), or zeros when not (g > 0).
`direct` is the same v taken straight from a loaded radiocore_oracle.Tuner's wideband spectrum, without the channel
samples (what the spectrum-direct route of rcfm_pipeline_run computes).  Channel signals of a wideband buffer come from
radiocore_oracle.Tuner (run_pruned), as the FM and AM tests take them; am_model.wideband places the stations.
"""

import numpy as np

from am_model import wideband  # noqa: F401  (re-exported: the band tests place SSB stations with it)

LEVEL = 0.25     # RCFM_SSB_LEVEL


def mask(B, lower):
    H = np.zeros(B)
    H[1:(B + 1) // 2] = 2.0
    return H[(-np.arange(B)) % B] if lower else H


def sideband(oracle, iq, B, A, lower):
    """v: the decimated sideband signal before the normalisation, float64 [A]."""
    x = np.asarray(iq).astype(np.complex64).astype(np.complex128)
    s = np.real(np.fft.ifft(mask(B, lower) * np.fft.fft(x)))
    return np.asarray(oracle.Decimate(B, A).run(s), np.float64)


def normalise(v):
    g = float(np.sqrt(np.mean(v * v)))
    if not g > 0:
        return np.zeros((len(v), 1))
    return np.clip(LEVEL * v / g, -0.999, 0.999)[:, None]


def expect(oracle, iq, B, A, lower):
    """Expected USB (lower=False) / LSB (lower=True) audio of one channel's samples iq (length B): float64 [A, 1]."""
    return normalise(sideband(oracle, iq, B, A, lower))


def expect_channel(oracle, ref_tuner, i, A, lower):
    """Expected audio of channel i of a loaded radiocore_oracle.Tuner."""
    iq = ref_tuner.run_pruned(i)
    return expect(oracle, iq, len(iq), A, lower)


def direct(oracle, Xw, roll, B, A, lower):
    """The same v from the Tuner's loaded spectrum Xw (length N, roll as radiocore_oracle.Tuner._roll gives it), A <= B <= N:
    bins +-k of the channel, the Tuner's Hann weight, Decimate's folded Hamming weight and Nyquist rule, one irfft."""
    N = len(Xw)
    k = np.arange(A // 2 + 1)
    q = -k if lower else k
    hann = oracle.shifted_window("hann", N)[q % N]
    W = oracle.shifted_window("hamm", B)
    Wr = np.where(k > 0, 0.5 * (W[k % B] + W[(B - k) % B]), W[0])
    Y = Xw[(q - roll) % N] * hann
    if lower:
        Y = np.conj(Y)
    Y = Y * Wr * (B / N)
    Y[k > (B - 1) // 2] = 0.0          # A == B, even: the bin B/2 is dropped
    Y[0] = 0.0
    if A % 2 == 0 and A < B:
        Y[A // 2] *= 2.0
    return np.fft.irfft(Y, A) * (A / B)


def ssb_iq(B, upper, lower, level=1.0, noise=0.0, seed=0):
    """Complex baseband with both sidebands occupied, complex128 [B]: tones (f Hz, amplitude a, phase p) in `upper`
    sit f above the channel centre, those in `lower` f below it (one-second buffer of B samples), plus complex white
    noise of standard deviation `noise` per component; everything times `level`."""
    t = np.arange(B, dtype=np.float64)
    x = np.zeros(B, np.complex128)
    for f, a, p in upper:
        x += a * np.exp(1j * (2 * np.pi * f * t / B + p))
    for f, a, p in lower:
        x += a * np.exp(-1j * (2 * np.pi * f * t / B + p))
    if noise:
        rng = np.random.default_rng(seed)
        x = x + noise * (rng.standard_normal(B) + 1j * rng.standard_normal(B))
    return level * x


def station_tones(i, seed=0):
    """Three tones per sideband, 300 .. 2700 Hz (the SSB voice band), amplitudes 0.5 .. 1 (6 dB), all six different."""
    rng = np.random.default_rng(1000 * seed + i)
    f = rng.choice(np.arange(300, 2701), 6, replace=False).astype(np.float64)
    a = rng.uniform(0.5, 1.0, 6)
    p = rng.uniform(0.0, 2 * np.pi, 6)
    tones = list(zip(f, a, p))
    return tones[:3], tones[3:]


def station(i, B, seed=0, noise=0.02, level=None):
    """Station i of a seeded band.  Levels spread over 14 dB unless `level` is given, so with the tones' 6 dB every
    sideband carries a signal within 20 dB of the strongest one in the buffer; the station's own noise floor is
    `noise` of its level (>= 1e-2 of either sideband's signal)."""
    rng = np.random.default_rng(5000 + 1000 * seed + i)
    drawn = 10.0 ** rng.uniform(-0.7, 0.0)
    upper, lower = station_tones(i, seed)
    return ssb_iq(B, upper, lower, drawn if level is None else level, noise, seed=7000 + 1000 * seed + i)


def band(N, f_in, centres, B, seed=0):
    """complex64 [N] buffer with station i centred at centres[i]."""
    return wideband(N, f_in, centres, B, [station(i, B, seed) for i in range(len(centres))], seed=seed)
