"""Carrier-estimate test model (no test functions): the definition of include/rcfm.h (rcfm_tuner_carriers) in float64,
the inputs the GPU tests use, and the float32 yardstick of the same definition.

For a channel with roll r and bandwidth B of an n-point spectrum X the bins are the signed offsets
d = -floor(B/2) .. -floor(B/2) + B - 1, bin d being X[(d - r) mod n], p_d = re^2 + im^2:
    peak_bin   = the d of the largest p_d (the lowest d among equals, a NaN never wins),  peak_power = that p_d / n^2
    centroid   = S1 / S0,  spread = sqrt(max(S2 / S0 - (S1 / S0)^2, 0)),  S_k = sum of d^k p_d over the bins with p_d >= G,
    G = float64(float32(gate)) n n;  centroid = spread = 0 when S0 is not positive.
The expectation takes X = numpy.fft.fft of the complex64 input in complex128; the yardstick takes scipy.fft.fft of the
complex64 input, which stays in single precision, forms p_d in float64 from its float32 parts as the device does and
rounds the results to float32, the format the entry point stores them in.

Tolerances -- YARDSTICK[case] = (centroid, spread): upper bounds of the yardstick's absolute error in bins, worst channel
of the case, measured by tests/test_carriers.py (figures beside each constant) and pinned one digit up; the device is held
to four times them (the convention of primitives_model.gpu_bound).  peak_bin is exact, peak_power within PEAK_POWER_REL,
the bound tests/test_hip_spectrum.py asserts for the same quantity (the square of one bin of the float32 transform).
"""

import numpy as np
import scipy.fft

PEAK_POWER_REL = 3e-5
GATE = 1e-6                 # the positive gate of every case, power per bin in the units of peak_power
SIDEBAND = 0.3              # each tone carries two sidebands of this relative amplitude (-10.5 dB), SIDE_BINS away:
SIDE_BINS = 40              #   the gated sums then run over two or three bins and the spread is well away from 0
SEG_BINS = 8192             # kernels.hip: bins per workgroup of a channel (level_segments)
MAX_SEGS = 64


# ---- the definition ---------------------------------------------------------------------------------------------------

def spectrum64(x):
    """The expectation's spectrum: numpy.fft.fft of the complex64 input taken to complex128."""
    assert x.dtype == np.complex64
    return np.fft.fft(x.astype(np.complex128))


def spectrum32(x):
    """The yardstick's spectrum: scipy.fft.fft of the complex64 input, complex64."""
    assert x.dtype == np.complex64
    X = scipy.fft.fft(x)
    assert X.dtype == np.complex64
    return X


def bins(n, roll, B):
    """(d, element index) of the B bins of a channel."""
    d = np.arange(B, dtype=np.int64) - B // 2
    return d, (d - int(roll)) % int(n)


def bin_power(X, n, roll, B):
    """(d, p_d) in float64; a complex64 spectrum contributes its float32 parts exactly."""
    d, idx = bins(n, roll, B)
    v = X[idx]
    return d, v.real.astype(np.float64) ** 2 + v.imag.astype(np.float64) ** 2


def gate_n2(gate, n):
    return float(np.float32(gate)) * float(n) * float(n)


def estimate(d, p, G, n):
    """(peak_bin, peak_power, centroid, spread) of one channel from its (d, p_d)."""
    valid = ~np.isnan(p)
    if valid.any():
        k = int(np.flatnonzero(valid & (p == np.max(p[valid])))[0])      # the lowest d among equals
        peak_bin, peak_power = int(d[k]), float(p[k]) / float(n) ** 2
    else:
        peak_bin, peak_power = int(d[0]), float("nan")
    with np.errstate(invalid="ignore"):
        on = p >= G
    dd = d[on].astype(np.float64)
    s0, s1, s2 = float(np.sum(p[on])), float(np.sum(dd * p[on])), float(np.sum(dd * dd * p[on]))
    if not s0 > 0.0:
        return peak_bin, peak_power, 0.0, 0.0
    m = s1 / s0
    return peak_bin, peak_power, m, float(np.sqrt(max(s2 / s0 - m * m, 0.0)))


def carriers(X, n, rolls, bws, gate):
    """The four arrays for channels (rolls[i], bws[i]): int64, float64, float64, float64."""
    G = gate_n2(gate, n)
    rows = [estimate(*bin_power(X, n, r, B), G, n) for r, B in zip(rolls, bws)]
    pb, pp, ce, sp = zip(*rows)
    return np.array(pb, np.int64), np.array(pp), np.array(ce), np.array(sp)


def yardstick(x, n, rolls, bws, gate):
    """The same definition on the single-precision transform, its results rounded to the float32 the entry point stores."""
    pb, pp, ce, sp = carriers(spectrum32(x), n, rolls, bws, gate)
    return pb, pp.astype(np.float32), ce.astype(np.float32), sp.astype(np.float32)


def honesty(X, n, rolls, bws, gate):
    """What keeps an exact comparison honest, from the model alone: (the smallest ratio in dB of a channel's strongest
    bin to its second strongest, the smallest |p_d / G - 1| over every bin of every channel; inf for gate 0)."""
    G = gate_n2(gate, n)
    lead, near = np.inf, np.inf
    for r, B in zip(rolls, bws):
        _, p = bin_power(X, n, r, B)
        if B > 1:
            top = np.partition(p, B - 2)[B - 2:]
            lead = min(lead, 10.0 * np.log10(top[1] / top[0]))
        if G > 0.0:
            near = min(near, float(np.min(np.abs(p / G - 1.0))))
    return float(lead), float(near)


# ---- the inputs -------------------------------------------------------------------------------------------------------

def segments(B):
    return min(MAX_SEGS, (B + SEG_BINS - 1) // SEG_BINS)


def boundary_offsets(B, head):
    """The tone offsets d that probe a channel of B bins whose run starts `head` (0 / 1) bins before a 16-byte boundary:
    the first and the last bin, both sides of every multiple of SEG_BINS bins, and both sides of every boundary between
    the workgroups' shares (the fast form deals out pairs of bins evenly, the general form bins)."""
    dlo, segs = -(B // 2), segments(B)
    out = {dlo, dlo + B - 1}
    for k in range(1, segs):
        e = k * SEG_BINS
        if e < B:
            out |= {dlo + e - 1, dlo + e}
        per_pairs = ((B - head) // 2 + segs - 1) // segs
        e = head + 2 * per_pairs * k
        if 0 < e < B:
            out |= {dlo + e - 1, dlo + e}
        per_bins = (B + segs - 1) // segs
        e = per_bins * k
        if e < B:
            out |= {dlo + e - 1, dlo + e}
    return sorted(out)


def band(n, chans, seed, noise=0.02, extra=()):
    """complex64 [n]: white noise (standard deviation `noise` per component) plus, for every channel
    (centre bin s, bandwidth, tone offset d, amplitude a), a tone at signed bin s + d with its two sidebands.
    extra: further (signed bin, amplitude) tones."""
    rng = np.random.default_rng(seed)
    X = np.zeros(n, np.complex128)
    for s, _, d, a in chans:
        X[(s + d) % n] += a * n
        X[(s + d + SIDE_BINS) % n] += SIDEBAND * a * n
        X[(s + d - SIDE_BINS) % n] += SIDEBAND * a * n
    for s, a in extra:
        X[s % n] += a * n
    x = np.fft.ifft(X) + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


def _amp(i):
    return 0.05 * 2.0 ** (i % 4 / 2.0)          # 0.05 .. 0.14, 3 dB apart


def case_fast():
    """N = 4 000 000, every channel in the fast form: B = 25 000 (4 workgroups), 12 500 (2), 2001 (odd), 7 (fewer bins
    than threads), each with even and odd base and a tone at every offset of boundary_offsets; a channel across signed
    bin 0 whose run starts in the front halo, one whose run ends in the back halo, one at each band edge."""
    n = 4_000_000
    chans = []
    s = -1_990_000
    for B in (25000, 12500, 2001, 7):
        for parity in (0, 1):
            head = (parity + B // 2) % 2          # element index of the run's first bin = base - B // 2, base = s mod n
            for d in (boundary_offsets(B, head) if B > 7 else [-3, 0, 3]):
                s += 26000
                s += (s % 2) != parity
                chans.append((s, B, d, _amp(len(chans))))
    assert s < -100_000
    chans += [(3, 25000, -7000, 0.2), (-5, 12500, 6000, 0.05),                  # front halo / back halo
              (n // 2 - 1, 25000, 12499, 0.2), (-(n // 2), 2001, -1000, 0.05),   # the band edges
              (200_000, 25000, 1234, 0.05)]
    return n, chans, band(n, chans, seed=11)


def case_odd(n):
    """The odd geometry of tests/test_hip_squelch.py (channels of 30 000 and 20 001 samples at rolls 7500 and -12 499) in
    n = 900 001 and n = 90 001, tones at a segment boundary and at the last bin."""
    chans = [(-7500, 30000, boundary_offsets(30000, 0)[3], 0.1), (12499, 20001, 10000, 0.07)]
    return n, chans, band(n, chans, seed=n % 89)


def case_general():
    """n = 90 001 and a channel with B = n: the handle keeps no halos and every channel takes the general form."""
    n = 90001
    chans = [(0, n, 31000, 0.5), (-20000, 2001, -1000, 0.05), (5000, 7, 3, 0.1), (30000, 12500, boundary_offsets(12500, 0)[4], 0.2)]
    return n, chans, band(n, chans, seed=5)


GRID_N, GRID_B, GRID_C, GRID_RASTER = 2_000_000, 25000, 24, 30000
GRID_OFFSETS = [0, 700, -1200, 3, -1, 2500, 0, -40, 911, -3000, 64, 1, -777, 1500, -2, 0, 350, -350, 1999, -1999, 5, 120, -64, 0]


def case_grid(seed=3):
    """What a Tuner over GRID_C channels of GRID_B on a 30 kHz raster reads (centres 100 MHz + 30 kHz (i - C / 2): the
    input frequency is 15 kHz below 100 MHz), one tone per channel, GRID_OFFSETS[i] bins off its centre."""
    chans = [(GRID_RASTER * (i - GRID_C // 2) + GRID_RASTER // 2, GRID_B, GRID_OFFSETS[i], 0.05 + 0.01 * (i % 5))
             for i in range(GRID_C)]
    return GRID_N, chans, band(GRID_N, chans, seed=seed)


CASES = {"fast": case_fast, "grid": case_grid, "odd900001": lambda: case_odd(900001), "odd90001": lambda: case_odd(90001),
         "general": case_general}
GATES = (0.0, GATE)

# (centroid, spread) of the float32 yardstick, absolute in bins, worst channel; key (case, gate > 0)
YARDSTICK = {
    ("fast", False): (4e-4, 5e-4),            # 3.63e-4, 4.45e-4
    ("fast", True): (5e-4, 3e-4),             # 4.67e-4, 2.89e-4
    ("grid", False): (9e-5, 4e-5),            # 8.33e-5, 3.68e-5
    ("grid", True): (1e-4, 1e-6),             # 9.59e-5, 9.25e-7
    ("odd900001", False): (3e-4, 5e-5),       # 2.87e-4, 4.39e-5
    ("odd900001", True): (3e-4, 2e-6),        # 2.38e-4, 1.32e-6
    ("odd90001", False): (5e-4, 6e-5),        # 4.33e-4, 5.50e-5
    ("odd90001", True): (3e-4, 5e-7),         # 2.93e-4, 4.53e-7
    ("general", False): (5e-4, 8e-4),         # 4.95e-4, 7.31e-4
    ("general", True): (2e-3, 7e-4),          # 1.18e-3, 6.29e-4
}

_cache = {}


def case(name):
    """(n, rolls, bws, x, X64) of a case, built once per process and not to be modified."""
    if name not in _cache:
        n, chans, x = CASES[name]()
        x.setflags(write=False)
        X = spectrum64(x)
        X.setflags(write=False)
        _cache[name] = (n, [-c[0] for c in chans], [c[1] for c in chans], x, X)
    return _cache[name]


def expected(name, gate):
    key = (name, "exp", float(gate))
    if key not in _cache:
        n, rolls, bws, _, X = case(name)
        _cache[key] = carriers(X, n, rolls, bws, gate)
    return _cache[key]


def gpu_bounds(name, gate):
    c, s = YARDSTICK[(name, gate > 0)]
    return 4.0 * c, 4.0 * s
