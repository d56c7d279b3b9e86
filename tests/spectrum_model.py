"""Wideband power spectrum test model (no test functions): the definition of include/rcfm.h
(rcfm_tuner_power_spectrum) in float64 on the complex64 input, the way squelch_model.py takes the oracle's float64
spectrum.

    P = |fftshift(fft(x as complex128))|^2 / N^2        signed bin s is P[s + N // 2]
    power[m] = sum, peak[m] = max of P over cell m of the span [s0, s0 + L), cells by radiocore.tools.spectrum.cell_edges
"""

import numpy as np

from radiocore.tools import spectrum


def shifted_power(x):
    """float64 [N]: |X|^2 / N^2 in ascending signed bin (ascending frequency); element i is signed bin i - N // 2."""
    x = np.asarray(x)
    X = np.fft.fftshift(np.fft.fft(x.astype(np.complex128)))
    return (X.real ** 2 + X.imag ** 2) / float(x.shape[0]) ** 2


def power_spectrum(P, s0, L, cells):
    """(power, peak), float64 [cells], of the span [s0, s0 + L) of shifted_power's P."""
    N = P.shape[0]
    assert -(N // 2) <= s0 and L >= 1 and s0 + L <= N - N // 2, (N, s0, L)
    span = P[s0 + N // 2: s0 + N // 2 + L]
    starts = spectrum.cell_edges(L, cells)[:-1]
    return np.add.reduceat(span, starts), np.maximum.reduceat(span, starts)


def noise_and_tones(N, seed=0):
    """complex64 [N]: complex white noise of 0.1 per component plus five tones of amplitude 0.05 * 0.7^i at signed bins
    -N//3, -7, 0, 12345 mod (N//2), N//2 - 3."""
    rng = np.random.default_rng(seed)
    x = 0.1 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    t = np.arange(N, dtype=np.float64) / N
    for i, s in enumerate((-(N // 3), -7, 0, 12345 % (N // 2), N // 2 - 3)):
        x += 0.05 * 0.7 ** i * np.exp(2j * np.pi * s * t)
    return x.astype(np.complex64)
