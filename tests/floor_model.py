"""The noise floor's definition (include/rcfm.h, "noise floor") in plain numpy: the ordering of float32 values, the sliding
order statistic with guard cells and shortened windows at the band ends, the rise / fall smoothing with its three float32
roundings, `over`, the thresholds -- the rank filter a second time cell by cell (`rank_filter_restated`), to pin the
vectorised form -- and the tilted-noise scene the Tuner tests run, with the margins their exact comparison rests on."""

import numpy as np

MARGIN_DB = 3.0          # the project's squelch margin: a model level this far from a threshold cannot be flipped by rounding
NAN_BITS = np.uint32(0x7fc00000)


def keys(x):
    """uint32 keys whose unsigned order is the ordering of include/rcfm.h: by value, -0 below +0, every NaN above +inf (and
    all NaNs equal)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where((u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000), np.uint32(0xffffffff), k).astype(np.uint32)


def values(k):
    """float32 of keys: the inverse of `keys`, NaN as 0x7fc00000."""
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k)
    return np.where(k == np.uint32(0xffffffff), NAN_BITS, u).astype(np.uint32).view(np.float32)


def counts(M, half, guard):
    """int64 [M]: the candidates of every cell, the cells j with 0 <= j < M and guard < |j - m| <= half."""
    m = np.arange(M, dtype=np.int64)
    return np.maximum(np.minimum(half, m) - guard, 0) + np.maximum(np.minimum(half, M - 1 - m) - guard, 0)


def ranks(cnt, q):
    """r = (q (cnt - 1)) / 1000 in 64-bit integers (0 where a cell has no candidate: unused)."""
    return (np.int64(q) * np.maximum(np.asarray(cnt, dtype=np.int64) - 1, 0)) // 1000


def _select(k, half, guard, q, sentinel):
    """The element of rank r among every cell's candidates, for sortable k [M]; `sentinel` sorts behind every value, and
    it stands for what is no candidate -- the cells beyond the band ends and the guard cells.  r < cnt, so it is never the
    answer of a cell that has a candidate."""
    M = k.shape[0]
    pad = np.full(half, sentinel, k.dtype)
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([pad, k, pad]), 2 * half + 1)
    r = ranks(counts(M, half, guard), q)
    out = np.empty(M, k.dtype)
    rows = max(1, (1 << 23) // (2 * half + 1))
    for a in range(0, M, rows):
        w = win[a:a + rows].copy()
        w[:, half - guard:half + guard + 1] = sentinel
        w.sort(axis=1)
        out[a:a + rows] = w[np.arange(w.shape[0]), r[a:a + rows]]
    return out


def rank_filter(x, half, guard, q):
    """float32 [M]: rcfm_rank_filter.  A cell without a candidate gets NaN."""
    k = keys(x)
    out = values(_select(k, half, guard, q, np.uint32(0xffffffff))).copy()     # (the sentinel ties with NaN: the same answer)
    out.view(np.uint32)[counts(k.shape[0], half, guard) == 0] = NAN_BITS
    return out


def rank_filter_restated(x, half, guard, q):
    """rank_filter as include/rcfm.h words it: cell by cell, the candidates collected by the index rule and sorted."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    k = keys(x)
    M = x.shape[0]
    out = np.empty(M, np.uint32)
    for m in range(M):
        cands = sorted(int(k[j]) for j in range(M) if guard < abs(j - m) <= half)
        if not cands:
            out[m] = NAN_BITS
            continue
        r = (q * (len(cands) - 1)) // 1000
        out[m] = values(np.array([cands[r]], np.uint32)).view(np.uint32)[0]
    return out.view(np.float32)


def rank_filter64(x, half, guard, q):
    """The same order statistic of float64 values without NaN (the Tuner tests' truth); a cell without a candidate: NaN."""
    x = np.asarray(x, dtype=np.float64)
    out = _select(x, half, guard, q, np.inf)
    out[counts(x.shape[0], half, guard) == 0] = np.nan
    return out


def smooth(state, e, rise, fall, dtype=np.float32):
    """s' of rcfm_floor_run: e where s is NaN, s where e is NaN, else s + a (e - s) with three roundings of `dtype`."""
    s, e = np.asarray(state, dtype=dtype), np.asarray(e, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(e > s, dtype(rise), dtype(fall)).astype(dtype)
        moved = (s + (a * (e - s)).astype(dtype)).astype(dtype)
    # (a NaN that the arithmetic itself makes, inf - inf, has the bits of whoever computed it: the tests keep clear of it)
    return np.where(np.isnan(s), e, np.where(np.isnan(e), s, moved)).astype(dtype)


def floor_run(state, power, half, guard, q, rise, fall, ratio):
    """(s' float32 [M], over uint8 [M]) of rcfm_floor_run from the state s and the buffer's power."""
    power = np.ascontiguousarray(power, dtype=np.float32)
    s = smooth(state, rank_filter(power, half, guard, q), rise, fall)
    with np.errstate(invalid="ignore", over="ignore"):
        over = power >= (np.float32(ratio) * s).astype(np.float32)
    return s, over.astype(np.uint8)


def thresholds(floor, cell, gain):
    """float32 [count]: rcfm_floor_thresholds -- floor[cell] gain, one float32 product; NaN for a cell outside [0, M)."""
    floor, cell = np.asarray(floor, dtype=np.float32), np.asarray(cell, dtype=np.int64)
    ok = (cell >= 0) & (cell < floor.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (floor[np.where(ok, cell, 0)] * np.asarray(gain, dtype=np.float32)).astype(np.float32)
    return np.where(ok, prod, np.float32(np.nan)).astype(np.float32)


def factor(tau):
    """a = 1 - exp(-1 / tau), 1 for tau = 0 (radiocore.tools.floor.smoothing_factor)."""
    return 1.0 if tau == 0 else -np.expm1(-1.0 / tau)


def channel_gain(B, n):
    """G(B, n) of include/rcfm.h's level definition, bin by bin: the sum of the squared weights a channel of bandwidth B reads
    its bins with -- W(k) = 0.5 - 0.5 cos(2 pi ((k - n // 2) mod n) / n) at k = 0 .. B // 2, at n - j for j = 1 .. B - B // 2 - 1,
    and for even B < n (B > 2) at n - B / 2 once more (that bin is added to +B / 2: independent bins, the squares add)."""
    def w2(k):
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * ((k - n // 2) % n) / n)) ** 2
    g = sum(w2(k) for k in range(0, B // 2 + 1)) + sum(w2(n - j) for j in range(1, B - B // 2))
    if B % 2 == 0 and 2 < B < n:
        g += w2(n - B // 2)
    return float(g)


# ---- the Tuner scene: tilted noise, stations over their local floor ----------------------------------------------------------

N, B, A, C = 40000, 2000, 800, 8
CELL_HZ, HALF, GUARD, QUANTILE = 100, 60, 12, 0.25
CELLS = N // CELL_HZ
SPACING = 4500                                    # the channels are spread over the band, so that they see most of the tilt
F_IN = 100.0e6
TILT_DB = 20.0
STATIONS = {0: 15.0, 1: 13.5, 3: 17.0}            # channel -> dB over the noise the channel holds (>= 13)
OVER_DB = 8.0


def centres():
    return [F_IN + SPACING * (i - (C - 1) / 2.0) for i in range(C)]


def tuner_setup(impl_tuner, demod):
    """add_channel / request_bandwidth of the scene on a Tuner of either implementation; demod(): a new demodulator.  The
    centres lie symmetrically around F_IN, which is therefore the input frequency."""
    t = impl_tuner
    for f in centres():
        t.add_channel(f, B, demod())
    t.request_bandwidth(float(N))
    return t


def density(scale=1.0):
    """float64 [N], fft order: the noise power per bin (E |X[k]|^2 / N^2), tilted by TILT_DB from the band's lower end to
    its upper end, times scale."""
    s = np.fft.fftfreq(N, 1.0 / N)                                    # signed bin of every fft bin
    return scale * 1e-8 * 10.0 ** (TILT_DB / 10.0 * (s + N // 2) / N)


def channel_bin(i):
    """The fft bin of channel i's centre."""
    return int(round(centres()[i] - F_IN)) % N


def buffer(seed, scale=1.0, stations=STATIONS):
    """complex64 [N]: noise shaped in the frequency domain to `density(scale)`, and in every channel of `stations` a carrier
    with two sidebands (at +-300 bins, a quarter of its amplitude) whose level is that many dB over the noise level the
    channel holds on average."""
    rng = np.random.default_rng(seed)
    d = density(scale)
    X = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(d / 2.0) * N
    for i, db in stations.items():
        k = channel_bin(i)
        noise = float(np.mean(d[(k + np.arange(-B // 2, B // 2)) % N])) * channel_gain(B, N)
        a = np.sqrt(noise * 10.0 ** (db / 10.0) / (1.0 + 2.0 / 16.0)) * N
        X[k] += a
        X[(k + 300) % N] += 0.25j * a
        X[(k - 300) % N] += 0.25j * a
    return np.fft.ifft(X).astype(np.complex64)


def cell_power64(x):
    """float64 [CELLS]: the power spectrum of the whole band in the floor's cells (rcfm_tuner_power_spectrum's definition,
    equal cells of CELL_HZ bins), from the float64 transform of the complex64 buffer."""
    X = np.fft.fftshift(np.fft.fft(np.asarray(x).astype(np.complex128)))
    p = (X.real ** 2 + X.imag ** 2) / float(N) ** 2
    return p.reshape(CELLS, CELL_HZ).sum(axis=1)


def channel_cells():
    """int64 [C]: the cell that holds every channel's centre bin."""
    return np.array([(int(round(f - F_IN)) + N // 2) // CELL_HZ for f in centres()], dtype=np.int64)


def gains(db):
    """float32 [C]: G(B) / len(cell) 10^(db / 10), float64 rounded once."""
    return np.full(C, channel_gain(B, N) / CELL_HZ * 10.0 ** (db / 10.0)).astype(np.float32)
