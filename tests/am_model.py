"""AM test model (no test functions): seeded AM signals and the expected audio of the AM demodulator.

The expectation follows include/rcfm.h (RCFM_AM) from the oracle's own pieces, in float64 after the float32 envelope:
    e = |x|;  v = radiocore_oracle.Decimate(B, A).run(e);  c = mean(v);
    audio = clip(v / c - 1, -0.999, 0.999), or zeros when not (c > 0).
Channel signals of a wideband buffer come from radiocore_oracle.Tuner (run_pruned), as the FM tests take them.
"""

import numpy as np


def message(B, tones, amps, phases=None):
    """Real modulating signal s[t] = sum a_k sin(2 pi f_k t / B + phi_k), scaled to peak 1 (one-second buffer of B
    samples, tones in Hz)."""
    t = np.arange(B, dtype=np.float64)
    phases = np.zeros(len(tones)) if phases is None else phases
    s = sum(a * np.sin(2 * np.pi * f * t / B + p) for f, a, p in zip(tones, amps, phases))
    return s / np.max(np.abs(s))


def am_iq(B, m, tones=(1000.0,), amps=(1.0,), phases=None, offset=0, level=1.0, noise=0.0, seed=0):
    """Complex baseband AM, complex128 [B]: level (1 + m s[t]) exp(2 pi j offset t / B) + complex white noise of
    standard deviation `noise` (relative to the carrier) per component."""
    s = message(B, tones, amps, phases)
    x = (1.0 + m * s) * np.exp(2j * np.pi * int(offset) * np.arange(B, dtype=np.float64) / B)
    if noise:
        rng = np.random.default_rng(seed)
        x = x + noise * (rng.standard_normal(B) + 1j * rng.standard_normal(B))
    return level * x


def station(i, B, seed=0, noise=0.01, level=None):
    """Station i of a seeded band: three tones in 300 .. 3400 Hz (the airband voice channel), modulation index
    0.3 .. 0.9, carrier up to +-1 kHz off the channel centre, and a level spread over 20 dB in amplitude (a power
    ratio of up to 100) unless `level` is given."""
    rng = np.random.default_rng(1000 * seed + i)
    tones = rng.uniform(300.0, 3400.0, 3).round()
    amps = rng.uniform(0.3, 1.0, 3)
    phases = rng.uniform(0.0, 2 * np.pi, 3)
    m = rng.uniform(0.3, 0.9)
    offset = int(rng.integers(-1000, 1001))
    drawn = 10.0 ** rng.uniform(-1.0, 0.0)
    level = drawn if level is None else level
    return am_iq(B, m, tones, amps, phases, offset, level, noise, seed=7000 + 1000 * seed + i)


def wideband(N, f_in, centres, B, stations, noise=1e-4, seed=0):
    """complex64 [N] buffer with stations[i] (complex [B]) centred at centres[i] (Hz, one-second buffer): its B-point
    spectrum added at bin offset int(f_c - f_in), scaled N / B so that the station keeps its time-domain amplitude."""
    Xw = np.zeros(N, np.complex128)
    kk = np.fft.fftfreq(B, 1.0 / B).astype(np.int64)
    for fc, x in zip(centres, stations):
        Xw[(kk + int(fc - f_in)) % N] += np.fft.fft(x) * (N / B)
    x = np.fft.ifft(Xw)
    del Xw
    rng = np.random.default_rng(seed + 11)
    x += noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return x.astype(np.complex64)


def expect(oracle, iq, B, A):
    """Expected AM audio of one channel's samples iq (length B): float64 [A, 1]."""
    e = np.abs(np.asarray(iq).astype(np.complex64)).astype(np.float32)
    v = np.asarray(oracle.Decimate(B, A).run(e), np.float64)
    c = float(np.mean(v))
    if not c > 0:
        return np.zeros((A, 1))
    return np.clip(v / c - 1.0, -0.999, 0.999)[:, None]


def expect_channel(oracle, ref_tuner, i, A):
    """Expected AM audio of channel i of a loaded radiocore_oracle.Tuner."""
    iq = ref_tuner.run_pruned(i)
    return expect(oracle, iq, len(iq), A)
