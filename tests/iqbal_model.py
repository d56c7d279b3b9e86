"""IQ balance test model (no test functions): the definitions of include/rcfm.h ("IQ balance": rcfm_tuner_iq_estimate,
rcfm_tuner_iq_correct) in float64 numpy -- estimate, finish, correct, notch, halos -- and the seeded input the CPU and GPU
tests share: a noise floor, a handful of noise-modulated stations at non-mirrored offsets 20 - 40 dB over it, impaired with
g = 1.05, phi = 3 degrees, plus a DC offset.
"""

import numpy as np

GAIN, PHASE = 1.05, np.deg2rad(3.0)
DC = 0.02 + 0.01j
QUALITY = 0.02           # the estimator's cap on the fixtures: |beta_hat - beta| <= QUALITY |beta|

# (offset, width, dB over the floor's density), offsets and widths as fractions of n.  No two stations mirror each other:
# the |offset| +- width / 2 intervals are disjoint.
STATIONS = [(+0.133, 0.044, 40.0), (-0.278, 0.067, 35.0), (+0.367, 0.033, 30.0), (-0.056, 0.022, 25.0), (+0.222, 0.017, 20.0)]

# The end-to-end band at n = 4 000 000: a wide station in the 240 kHz channel at +1.2 MHz and narrow ones in the 12.5 kHz
# channels at -300, +312.5 and -337.5 kHz; every mirror channel is empty (E2E_CHANNELS: offsets from the input frequency).
E2E_N = 4_000_000
E2E_STATIONS = [(+0.3, 0.05, 30.0), (-0.075, 0.0025, 40.0), (+0.078125, 0.0025, 35.0), (-0.084375, 0.0025, 25.0)]
E2E_CHANNELS = [(-1_200_000, 240000), (+1_200_000, 240000)] + \
               [(sign * (300_000 + 12_500 * i), 12500) for i in range(4) for sign in (-1, +1)]

# name: (n, seed, stations) of every input the GPU tests load
FIXTURES = {"odd": (90001, 11, STATIONS), "even": (600000, 12, STATIONS), "fast": (E2E_N, 13, E2E_STATIONS),
            "nohalo": (100000, 14, STATIONS), "rocfft": (10007, 15, STATIONS)}


def fixture(name):
    """complex128 [n]: the received (impaired, DC-offset) buffer of FIXTURES[name]."""
    n, seed, stations = FIXTURES[name]
    return received(n, seed, stations)


def receiver(gain=GAIN, phase=PHASE):
    """(mu, nu, beta): x' = mu x + nu conj(x), beta = nu / conj(mu)."""
    mu = (1.0 + gain * np.exp(-1j * phase)) / 2.0
    nu = (1.0 - gain * np.exp(1j * phase)) / 2.0
    return complex(mu), complex(nu), complex(nu / np.conj(mu))


def impair(x, gain=GAIN, phase=PHASE):
    mu, nu, _ = receiver(gain, phase)
    x = np.asarray(x, np.complex128)
    return mu * x + nu * np.conj(x)


def station_bins(n, stations):
    """[(first signed bin, width in bins, dB)] of fractional stations in an n-bin spectrum."""
    out = []
    for off, width, db in stations:
        w = max(int(round(width * n)), 1)
        out.append((int(round(off * n)) - w // 2, w, db))
    return out


def clean_band(n, seed, stations=STATIONS, carriers=(), rms=0.2):
    """complex128 [n], the true baseband: white noise plus band-limited Gaussian noise per station (a station whose
    modulation fills its width), plus unmodulated carriers [(signed bin, dB over the floor's density)], scaled to `rms`."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    for s0, w, db in station_bins(n, stations):
        k = (s0 + np.arange(w)) % n
        X[k] += 10.0 ** (db / 20.0) * (rng.standard_normal(w) + 1j * rng.standard_normal(w)) / np.sqrt(2.0)
    for s, db in carriers:
        X[int(s) % n] += 10.0 ** (db / 20.0) * np.exp(2j * np.pi * rng.uniform())
    x = np.fft.ifft(X)
    return x * (rms / np.sqrt(np.mean(np.abs(x) ** 2)))


def received(n, seed, stations=STATIONS, carriers=(), dc=DC):
    """complex128 [n]: clean_band through the impaired receiver, plus its DC offset."""
    return impair(clean_band(n, seed, stations, carriers)) + dc


def quantise_cu8(x):
    """uint8 [n, 2]: what an RTL-SDR delivers for x (full scale 1.0, centre 127.5), clipped."""
    v = np.stack([x.real, x.imag], axis=-1) * 128.0 + 127.5
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def quantise_cs16(x):
    v = np.stack([x.real, x.imag], axis=-1) * 32768.0
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def from_cu8(raw):
    raw = np.asarray(raw).reshape(-1, 2).astype(np.float64)
    return ((raw[:, 0] - 127.5) + 1j * (raw[:, 1] - 127.5)) / 128.0


def from_cs16(raw):
    raw = np.asarray(raw).reshape(-1, 2).astype(np.float64)
    return (raw[:, 0] + 1j * raw[:, 1]) / 32768.0


# ---- the definitions ---------------------------------------------------------------------------------------------------

def mirror(n):
    """int64 [n]: k' = (n - k) mod n."""
    return (n - np.arange(n, dtype=np.int64)) % n


def last_pair(n):
    return (n - 1) // 2


def estimate_sums(X, m_lo=1, m_hi=None):
    """(sums, cross): sums = float64 [3] Re P, Im P, Q over the pairs m_lo .. m_hi of X (any complex dtype, promoted to
    float64), cross = sum |X[m]| |X[n - m]|, the scale of P's bound."""
    X = np.asarray(X).astype(np.complex128)
    n = X.shape[0]
    m_hi = last_pair(n) if m_hi is None else m_hi
    if not (1 <= m_lo <= m_hi <= last_pair(n)):
        raise ValueError("pairs [%d, %d] outside [1, %d]" % (m_lo, m_hi, last_pair(n)))
    m = np.arange(m_lo, m_hi + 1, dtype=np.int64)
    a, b = X[m], X[n - m]
    P = np.sum(a * b)
    Q = np.sum(a.real ** 2 + a.imag ** 2 + b.real ** 2 + b.imag ** 2)
    return np.array([P.real, P.imag, Q]), float(np.sum(np.abs(a) * np.abs(b)))


def finish(sums):
    """beta (complex, float64) of Re P, Im P, Q: c = 2 P / Q, beta = c / (1 + sqrt(1 - min(|c|^2, 1))); 0 for Q = 0 or
    anything non-finite."""
    pr, pi, q = (float(v) for v in sums)
    if not (q > 0.0 and np.isfinite(pr) and np.isfinite(pi) and np.isfinite(q)):
        return 0j
    cr, ci = (2.0 * pr) / q, (2.0 * pi) / q
    d = 1.0 + np.sqrt(1.0 - min(cr * cr + ci * ci, 1.0))
    beta = complex(cr / d, ci / d)
    return beta if np.isfinite(beta.real) and np.isfinite(beta.imag) else 0j


def finish_f32(sums):
    """(re, im) float32: the finish rounded once."""
    b = finish(sums)
    return np.float32(b.real), np.float32(b.imag)


def notch_bins(n, w):
    """The bins of signed index |s| <= w - 1."""
    if w <= 0:
        return np.zeros(0, np.int64)
    s = np.arange(-(w - 1), w, dtype=np.int64)
    return np.unique(s % n)


def correct(X, beta, notch=0):
    """complex128 [n]: Y[k] = X[k] - beta conj(X[k']), then the notch."""
    X = np.asarray(X).astype(np.complex128)
    n = X.shape[0]
    Y = X - complex(beta) * np.conj(X[mirror(n)])
    Y[notch_bins(n, notch)] = 0.0
    return Y


def correct_bound(X, beta):
    """float64 [n]: 6 2^-24 (|X[k]| + |beta| |X[k']|), the elementwise bound of the float32 correction."""
    X = np.asarray(X).astype(np.complex128)
    return 6.0 * 2.0 ** -24 * (np.abs(X) + abs(complex(beta)) * np.abs(X[mirror(X.shape[0])]))


def with_halos(Y, halo):
    """[halo | n | halo]: the halos repeat the far ends."""
    n = Y.shape[0]
    return np.concatenate([Y[n - halo:], Y, Y[:halo]]) if halo else Y.copy()


def balance(X, notch=0, m_lo=1, m_hi=None):
    """(Y, beta): the auto mode on one spectrum."""
    beta = finish(estimate_sums(X, m_lo, m_hi)[0])
    return correct(X, beta, notch), beta
