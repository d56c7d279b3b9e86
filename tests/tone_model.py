"""The tone bank and the tone score as include/rcfm.h defines them ("tone bank"), in float64 -- and a float32 yardstick of
the same sums, for the GPU tests' error bound: float32 phasor tables rounded once from float64, float32 products and
numpy's float32 sums.  numpy only."""

import numpy as np


def rows(audio, step=1, offset=0):
    """[C, A] view of audio [C, A step] or [C, A, step]: sample i of a channel is element i step + offset of its row."""
    a = np.asarray(audio)
    a = a.reshape(a.shape[0], -1)
    return a[:, offset::step]


def hann(L):
    """The periodic Hann window radiocore.ToneBank uses, float32 [L]."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L, dtype=np.float64) / L)).astype(np.float32)


def phasors(nu, L):
    """complex128 [K, L]: exp(-2 pi j frac(nu[k] i)), the product and its fraction in float64."""
    t = np.asarray(nu, dtype=np.float64)[:, None] * np.arange(L, dtype=np.float64)[None, :]
    return np.exp(-2j * np.pi * (t - np.floor(t)))


def _frames(audio, L, step, offset):
    x = rows(audio, step, offset)
    C, A = x.shape
    if A < L:
        raise ValueError("the audio row is shorter than one frame")
    F = A // L
    return x[:, :F * L].reshape(C, F, L)


def tone_bank(audio, nu, L, window=None, step=1, offset=0):
    """(P [C, F, K], E [C, F]) in float64 from the float32 audio and window."""
    x = _frames(audio, L, step, offset).astype(np.float64)
    w = np.ones(L) if window is None else np.asarray(window, dtype=np.float32).astype(np.float64)
    S = float(np.sum(w))
    Z = np.einsum("cfl,kl->cfk", x * w, phasors(nu, L)) / S
    return np.abs(Z) ** 2, np.mean(x * x, axis=2)


def tone_bank_f32(audio, nu, L, window=None, step=1, offset=0):
    """The float32 yardstick: the same sums with float32 tables, products and numpy float32 sums."""
    x = _frames(audio, L, step, offset).astype(np.float32)
    w = np.ones(L, np.float32) if window is None else np.asarray(window, dtype=np.float32)
    S = np.float32(np.sum(w.astype(np.float64)))
    e = phasors(nu, L)
    er, ei = e.real.astype(np.float32), e.imag.astype(np.float32)
    t = x * w
    K = er.shape[0]
    P = np.empty(x.shape[:2] + (K,), np.float32)
    for k in range(K):
        zr = np.sum(t * er[k], axis=2, dtype=np.float32) / S
        zi = np.sum(t * ei[k], axis=2, dtype=np.float32) / S
        P[:, :, k] = zr * zr + zi * zi
    E = np.sum(x * x, axis=2, dtype=np.float32) / np.float32(L)
    return P, E


def largest_power(audio, L, window=None, step=1, offset=0):
    """float64 [C, F]: (sum_i |w_i x_i| / S)^2, the largest value P can take for that frame -- the error's denominator."""
    x = _frames(audio, L, step, offset).astype(np.float64)
    w = np.ones(L) if window is None else np.asarray(window, dtype=np.float32).astype(np.float64)
    return (np.sum(np.abs(x * w), axis=2) / float(np.sum(w))) ** 2


def tone_score(P, E, want, gate=None):
    """float64 [C]: max_f P[c, f, want[c]] / E[c, f], frames with E == 0 contributing 0; +inf for want == -1; NaN where
    gate == 0 (whatever want is) and for a want outside [-1, K)."""
    P, E = np.asarray(P, dtype=np.float64), np.asarray(E, dtype=np.float64)
    C, F, K = P.shape
    out = np.empty(C)
    for c in range(C):
        k = int(want[c])
        if (gate is not None and not gate[c]) or k < -1 or k >= K:
            out[c] = np.nan
        elif k == -1:
            out[c] = np.inf
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(E[c] == 0, 0.0, P[c, :, k] / E[c])
            out[c] = max(0.0, np.nanmax(r)) if not np.all(np.isnan(r)) else 0.0
    return out


def open_mask(score, ratio):
    """The rcfm_squelch rule on a score: open iff score >= ratio, false for NaN."""
    with np.errstate(invalid="ignore"):
        return np.asarray(score) >= np.asarray(ratio)


def margin(score, ratio):
    """How many times the nearest finite, non-zero score lies away from its threshold (>= 1; inf without such a score)."""
    s = np.asarray(score, dtype=np.float64)
    r = np.broadcast_to(np.asarray(ratio, dtype=np.float64), s.shape)
    ok = np.isfinite(s) & (s > 0)
    if not ok.any():
        return np.inf
    q = s[ok] / r[ok]
    return float(np.min(np.maximum(q, 1.0 / q)))


def speech(rng, A, sigma=0.2):
    """Noise-like "speech": white Gaussian of standard deviation sigma, float64 [A]."""
    return sigma * rng.standard_normal(A)


def tone(A, freq_hz, amplitude, phase=0.0):
    """One second of a sinusoid at freq_hz sampled A times, float64 [A]."""
    return amplitude * np.cos(2.0 * np.pi * freq_hz * np.arange(A, dtype=np.float64) / A + phase)
