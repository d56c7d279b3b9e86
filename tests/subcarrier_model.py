"""The subcarrier tap (include/rcfm.h, rcfm_subcarrier_*): float64 truth, a float32 restatement, the case tables and the
tolerances (no test functions; CPU only).

Truth -- truth(x, R, f, h): the definition of include/rcfm.h on the complex64 input cast UP: d = signal_edges.steps (the
phase step / pi in float64, d[0] = 0), times exp(-2 pi i ((n f) mod B) / B) with the product in exact integers, then the
LINEAR correlation with h (zero extension) at every D-th sample.

Yardstick -- f32(x, R, f, h): the same in float32 the way the library evaluates it: float32 angle / pi, the wrapped
difference, g[i] = h[i] exp(..) and rot[j] formed in float64 and stored as complex64, one complex64 accumulator per output
fed tap after tap, times rot in complex64.  tests/test_subcarrier_model.py evaluates its error against the truth for every
case and asserts it below the constant pinned here (measured plus a quarter, the rule of primitives_model.YARDSTICK); the
device is held to primitives_model.gpu_bound(constant) = min(4 x constant, 1e-4).  Nothing a kernel returns enters them.

Metric -- primitives_model.row_errors: max|delta| / max|truth| per channel, worst channel, no sample left out.
Inputs -- primitives_model.discriminator_input: phase steps within +-0.85 pi, row amplitudes over three decades, each row
beginning 0.7 pi beyond the end of the one before (a difference taken across rows would show).
"""

import functools

import numpy as np

import primitives_model as pm
import rds_model
import signal_edges
import tuner_model

ROWS = 3
# (B, R, f, T): float32 yardstick (the figure test_subcarrier_model.py prints, plus a quarter).  Every comment names the
# tile the kernel takes for the case's D = B / R and T, "J = <outputs per workgroup>" (0: the single-output kernel), as
# rcfm_subcarrier_describe reports it: test_subcarrier_model.py holds the comments to the library and the table to every J.
CASES = {
    (240000, 9600, 57000, 241): 1.09e-6,   # 64-bit phase index, D = 25 (RDS), J = 256 [measured 8.72e-7]
    (12500, 500, 100, 151): 4.0e-7,        # a CTCSS tone of a narrow channel, D = 25, J = 256 [measured 3.22e-7]
    (6000, 6000, 0, 1): 2.8e-7,            # D = 1, one tap: y = d + 0j, J = 1024 [measured 2.26e-7]
    (6000, 240, 2999, 257): 7.6e-7,        # f next to B / 2, T > D, D = 25, J = 256 [measured 6.07e-7]
    (1000, 200, -300, 31): 2.4e-7,         # negative f, D = 5, J = 1024 [measured 1.94e-7]
    (1001, 91, 77, 15): 2.0e-7,            # odd B: rows only 8-byte aligned, D = 11, J = 512 [measured 1.63e-7]
    (6000, 1, 1234, 4095): 2.0e-6,         # one output, the longest filter, D = 6000 > T, J = 0 [measured 1.6e-6]
    # every other tile, the deepest rows, the ragged last tiles and the mixed store paths
    (12000, 6000, 1500, 4095): 2.8e-6,     # D = 2, J = 1024: rpad = 2048, 512 steps per row, a third of the outputs over a row end [measured 2.23e-6; MI355X 1.85e-6]
    (12000, 4000, -2000, 257): 1.03e-6,    # D = 3, J = 1024: D does not divide the staging group of four samples [measured 8.27e-7; MI355X 6.19e-7]
    (12500, 125, 1000, 241): 6.0e-7,       # D = 100, J = 128: half a wave computes, 125 of 128 outputs, R % 4 = 1 [measured 4.79e-7; MI355X 4.79e-7]
    (20000, 100, 3000, 241): 5.85e-7,      # D = 200, J = 64: 16 lanes compute, second tile 36 of 64 [measured 4.68e-7; MI355X 4.96e-7]
    (20000, 80, 3000, 241): 6.05e-7,       # D = 250, J = 32: three tiles, the last one 16 of 32 [measured 4.85e-7; MI355X 5.50e-7]
    (24000, 48, 5000, 241): 4.7e-7,        # D = 500 > T, J = 16: one step per row, rows from T on carry no tap [measured 3.76e-7; MI355X 3.15e-7]
    (20000, 20, 7000, 241): 6.35e-7,       # D = 1000, J = 8: the last tile 4 of 8 [measured 5.07e-7; MI355X 5.79e-7]
    (27300, 20, 9000, 241): 3.55e-7,       # D = 1365, J = 4: the last tile that fits (65 520 bytes), one computing thread [measured 2.84e-7; MI355X 2.81e-7]
    (27320, 20, 9000, 241): 4.1e-7,        # D = 1366, J = 0: its neighbour, the single-output kernel with T < 256 [measured 3.30e-7; MI355X 1.32e-7]
    (24000, 24, -7000, 4095): 1.47e-6,     # D = 1000 < T, J = 4: rpad = 8 at the smallest tile, negative f [measured 1.18e-6; MI355X 1.67e-6]
    (8190, 6, 100, 31): 2.6e-7,            # D = 1365, J = 4: R % 4 = 2 under 16-byte stores, the last tile holds 2 outputs [measured 2.09e-7; MI355X 1.37e-7]
    (12500, 250, 19, 151): 3.55e-7,        # D = 50, J = 256: R % 4 = 2, one tile, its last computing lane stores 2 outputs [measured 2.84e-7; MI355X 3.59e-7]
}
# the cases whose row ends test_hip_subcarrier.py reports apart from the interior (edge_outputs)
EDGE_CASES = ((12000, 6000, 1500, 4095), (6000, 240, 2999, 257))
# a Tuner whose channels have a prime bandwidth (no engine plan: rocFFT, samples instead of phases): (n, B, R, f, T)
PRIME_BAND = (90000, 3001, 3001, 700, 31)      # D = 1, J = 1024
PRIME_BAND_YARDSTICK = 1.45e-6          # measured 8.9e-7, 1.16e-6, 9.5e-7 on the three channels
# two bands whose channels the engine plans (the Tuner hands over phases, k_subcarrier_tap<true>), built like the prime band
PHASE_BAND_ONE = (100000, 12500, 125, 1000, 241)   # D = 100, J = 128: phase rows 16-byte aligned
PHASE_BAND_ONE_YARDSTICK = 5.4e-7       # measured 2.4e-7, 4.3e-7, 4.3e-7 on the three channels; MI355X 5.2e-7, 8.4e-7, 7.6e-7
PHASE_BAND_TWO = (81000, 10125, 81, 700, 31)       # D = 125, J = 64: B odd, phase rows only 4-byte aligned (scalar loads)
PHASE_BAND_TWO_YARDSTICK = 3.7e-7       # measured 1.5e-7, 3.0e-7, 1.4e-7 on the three channels; MI355X 2.2e-7, 2.3e-7, 1.7e-7
# the three RDS stations of rds_model.band() through the Tuner: R, f, T, cutoff; one yardstick per channel
RDS_TAP = (9600, 57000, 241, 3000.0)           # B = 240 000, D = 25, J = 256
RDS_YARDSTICK = (2.45e-6, 3.55e-6, 4.2e-6)     # measured 1.95e-6, 2.82e-6, 3.35e-6 (amplitudes 0.3, 0.1, 0.06)


def taps(T):
    """Unit-DC-gain Hamming low-pass at 0.2 of Nyquist, float32 (T = 1: the identity)."""
    return pm.filter_taps("firwin", T)


def rds_taps(B, R, T, cutoff):
    """radiocore.tools.rds.taps restated: Hamming windowed sinc, -6 dB at `cutoff` Hz, unit DC gain, float32."""
    del R
    m = np.arange(T) - 0.5 * (T - 1)
    h = np.sinc(2.0 * cutoff / B * m) * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(T) / (T - 1)))
    return (h / np.sum(h)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_input(B, seed=11):
    x = pm.discriminator_input(ROWS, B, seed)
    x.setflags(write=False)
    return x


def mixer(k, f, B):
    """exp(-2 pi i ((k f) mod B) / B) in float64, the product in exact integers (k: int64 array)."""
    r = (np.asarray(k, np.int64) * int(f)) % int(B)
    return np.exp(-2j * np.pi * r / float(B))


def discriminator(x):
    """[C][B] float64: signal_edges.steps per row."""
    return np.array([signal_edges.steps(row) for row in np.atleast_2d(x)])


def truth(x, R, f, h):
    """[C][R] complex128 from x [C][B] (any complex dtype, cast up)."""
    x = np.atleast_2d(x)
    B, T = x.shape[1], len(h)
    D, c = B // R, (len(h) - 1) // 2
    assert B % R == 0 and T % 2 == 1
    m = discriminator(x) * mixer(np.arange(B), f, B)
    h64 = np.asarray(h, np.float64)
    # sum_i h[i] m[jD + i - c] = convolve(m, reversed h)[jD + c]
    return np.array([np.convolve(row, h64[::-1])[c:c + B:D][:R] for row in m])


def truth_loops(x, R, f, h):
    """The definition as a literal double loop (small B only)."""
    x = np.atleast_2d(x)
    B, T = x.shape[1], len(h)
    D, c = B // R, (T - 1) // 2
    d = discriminator(x)
    y = np.zeros((x.shape[0], R), np.complex128)
    for row in range(x.shape[0]):
        for j in range(R):
            for i in range(T):
                n = j * D + i - c
                if 0 <= n < B:
                    y[row, j] += float(h[i]) * d[row, n] * np.exp(-2j * np.pi * ((n * int(f)) % B) / B)
    return y


def f32(x, R, f, h):
    """[C][R] complex64: the library's evaluation form in float32 / complex64 (module docstring)."""
    x = np.atleast_2d(np.asarray(x, np.complex64))
    C, B = x.shape
    T = len(h)
    D, c = B // R, (T - 1) // 2
    th = np.angle(x) / np.float32(np.pi)
    assert th.dtype == np.float32
    step = th[:, 1:] - th[:, :-1]
    step = step - np.float32(2.0) * np.rint(np.float32(0.5) * step)
    d = np.zeros((C, B + 2 * T), np.float32)                 # zero extension on both sides
    d[:, T + 1:T + B] = step
    g = (np.asarray(h, np.float64) * mixer(np.arange(T) - c, f, B)).astype(np.complex64)
    rot = mixer(np.arange(R, dtype=np.int64) * D, f, B).astype(np.complex64)
    acc = np.zeros((C, R), np.complex64)
    start = T - c + D * np.arange(R)
    for i in range(T):
        acc += g[i] * d[:, start + i]
    y = acc * rot
    assert y.dtype == np.complex64
    return y


# ---- the Tuner cases ----------------------------------------------------------------------------------------------------------

def _rolls(f_in, centres):
    return [int(f_in - fc) for fc in centres]


@functools.lru_cache(maxsize=None)
def rds_channels():
    """(float64 channels [3][B], float32-model channels [3][B] complex64) of rds_model.band() through tuner_model."""
    import scipy.fft
    x = rds_model.band()
    n, B = rds_model.N, rds_model.B
    rolls = _rolls(rds_model.input_frequency(), rds_model.CENTRES)
    X64 = np.fft.fft(x.astype(np.complex128))
    X32 = scipy.fft.fft(x)
    assert X32.dtype == np.complex64
    ref = np.array([tuner_model.ref_channel(X64, n, r, B) for r in rolls])
    low = np.array([tuner_model.f32_channel(X32, n, r, B) for r in rolls])
    return ref, low


@functools.lru_cache(maxsize=None)
def rds_truth():
    """[3][R] complex128, read-only: the tap of the three stations, float64 from the wideband buffer on."""
    R, f, T, cutoff = RDS_TAP
    y = truth(rds_channels()[0], R, f, rds_taps(rds_model.B, R, T, cutoff))
    y.setflags(write=False)
    return y


def band_centres(B):
    return [1e6 - 3 * B, 1e6, 1e6 + 3 * B]


@functools.lru_cache(maxsize=None)
def small_band(n, B):
    """(x [n] complex64, f_in, centres): three channels of bandwidth B, each a smooth FM station (signal_edges.dc_station
    at level 0: tones of 0.12 at 300 .. 1102 Hz, one of them at or next to the tap frequency of every band here)."""
    centres = band_centres(B)
    f_in = 0.5 * (min(centres) + max(centres))
    st = [signal_edges.dc_station(B, i, 0.0) for i in range(len(centres))]
    x = signal_edges.wideband_from(st, n, f_in, centres, B, gain=(0.3, 0.1, 0.2))
    x.setflags(write=False)
    return x, f_in, centres


@functools.lru_cache(maxsize=None)
def small_band_channels(n, B):
    """(float64 channels [3][B], float32-model channels [3][B] complex64) of small_band(n, B) through tuner_model."""
    import scipy.fft
    x, f_in, centres = small_band(n, B)
    rolls = _rolls(f_in, centres)
    X64 = np.fft.fft(x.astype(np.complex128))
    X32 = scipy.fft.fft(x)
    ref = np.array([tuner_model.ref_channel(X64, n, r, B) for r in rolls])
    low = np.array([tuner_model.f32_channel(X32, n, r, B) for r in rolls])
    return ref, low


@functools.lru_cache(maxsize=None)
def small_band_truth(band):
    """[3][R] complex128, read-only: the tap of band = (n, B, R, f, T), float64 from the wideband buffer on."""
    n, B, R, f, T = band
    y = truth(small_band_channels(n, B)[0], R, f, taps(T))
    y.setflags(write=False)
    return y


def prime_band_centres():
    return band_centres(PRIME_BAND[1])


def prime_band():
    return small_band(*PRIME_BAND[:2])


def prime_band_channels():
    return small_band_channels(*PRIME_BAND[:2])


def edge_outputs(B, R, T):
    """How many outputs at a row's head reach in front of sample 1 (j D - c < 1; at its tail one fewer reaches past the
    end, j D - c + T > B): the `edge` of primitives_model.segment_errors, whose tail takes one interior output along."""
    return ((T - 1) // 2) // (B // R) + 1
