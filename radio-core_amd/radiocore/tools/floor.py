"""NoiseFloor: an OS-CFAR noise floor on the Tuner's power spectrum, tracked from buffer to buffer on the device and turned
into per-channel thresholds there (rcfm_rank_filter / rcfm_floor_*, include/rcfm.h; no reference counterpart).
``Tuner.set_floor`` runs one behind every load; ``OverFloor(db)`` then stands where ``set_squelch`` and ``set_gate`` take a
threshold: "db over the floor, here and now", without a calibration pass."""

import ctypes
import math

import numpy as np

from radiocore._internal import hip

__all__ = ["NoiseFloor", "OverFloor", "channel_noise_gain"]


class OverFloor:
    """``OverFloor(db)``: a threshold ``db`` dB over the noise floor at the channel, as the last load tracked it.  It stands
    where ``Tuner.set_squelch`` and ``Tuner.set_gate`` take a level and needs ``Tuner.set_floor``."""

    def __init__(self, db):
        db = float(db)
        if not math.isfinite(db):
            raise ValueError("OverFloor: a finite number of dB, not %r" % (db,))
        self.db = db

    def __repr__(self):
        return "OverFloor(%g)" % self.db


def smoothing_factor(tau):
    """a = 1 - exp(-1 / tau) for a time constant of tau seconds at one buffer per second; tau = 0: a = 1, no memory."""
    tau = float(tau)
    if not math.isfinite(tau) or tau < 0.0:
        raise ValueError("a time constant is seconds, finite and at least 0, not %r" % (tau,))
    return 1.0 if tau == 0.0 else -math.expm1(-1.0 / tau)


class NoiseFloor:
    """``NoiseFloor(cell_hz, half=64, guard=4, quantile=0.25, rise=10.0, fall=1.0)``: the band is cut into cells of
    ``cell_hz`` Hz (``Tuner.power_spectrum``'s cells over the whole band); the floor estimate of a cell is the ``quantile``
    of the up to ``2 (half - guard)`` cells within ``half`` cells of it, the ``guard`` cells next to it on either side left
    out (a station wider than a cell does not raise its own floor), with a shorter window at the band ends.  The estimate
    of each buffer moves the tracked floor with the time constant ``rise`` (seconds; upwards: slow, a transmission that
    fills the window does not drag the floor up at once) or ``fall`` (downwards: fast); 0 means no memory.  Buffers are
    one second long."""

    def __init__(self, cell_hz, half=64, guard=4, quantile=0.25, rise=10.0, fall=1.0):
        cell_hz = float(cell_hz)
        if not math.isfinite(cell_hz) or cell_hz < 1.0:
            raise ValueError("cell_hz: at least one bin (1 Hz), not %r" % (cell_hz,))
        if int(half) != half or not 1 <= int(half) <= hip.RCFM_FLOOR_MAX_HALF:
            raise ValueError("half: an integer from 1 to %d, not %r" % (hip.RCFM_FLOOR_MAX_HALF, half))
        if int(guard) != guard or not 0 <= int(guard) <= int(half) - 1:
            raise ValueError("guard: an integer from 0 to half - 1, not %r" % (guard,))
        quantile = float(quantile)
        if not 0.0 <= quantile <= 1.0:
            raise ValueError("quantile: from 0 to 1, not %r" % (quantile,))
        self.cell_hz = cell_hz
        self.half = int(half)
        self.guard = int(guard)
        self.quantile = quantile
        self.rise = float(rise)
        self.fall = float(fall)
        self.factors                     # (raises for a bad time constant)

    @property
    def q(self):
        """The quantile in thousandths, the rank rule's q."""
        return int(round(1000.0 * self.quantile))

    @property
    def factors(self):
        """(rise, fall) as the float32 smoothing factors the device applies."""
        return np.float32(smoothing_factor(self.rise)), np.float32(smoothing_factor(self.fall))

    def cells(self, n):
        """Cells of the whole band of an n-sample buffer: ``max(1, round(n / cell_hz))``."""
        return max(1, int(round(int(n) / self.cell_hz)))

    def _create(self, M):
        """A new librcfm handle (no cell primed) for M cells."""
        a, b = self.factors
        out = ctypes.c_void_p()
        lib = hip.lib()
        hip.check(lib.rcfm_floor_create(int(M), self.half, self.guard, self.q, float(a), float(b), ctypes.byref(out)))
        return hip.Handle(out, lib.rcfm_floor_destroy)


def channel_noise_gain(B, n):
    """G: what ``Tuner.levels()`` reads, on average, for a channel of bandwidth B <= n over white noise of unit power per
    bin (E |X[k]|^2 / n^2 = 1) in an n-sample buffer, float64.  The level is the sum of |w X|^2 over the channel's bins,
    w the fftshifted periodic Hann window of length n at the bin's distance k from the channel centre,
    W(k) = 0.5 - 0.5 cos(2 pi (k - n // 2) / n): bins 0 .. B // 2 above, B - B // 2 - 1 below, and for even B < n
    (B > 2) the bin -B/2, which is added to bin +B/2 before squaring -- independent bins, so the squares still add."""
    B, n = int(B), int(n)
    if not 1 <= B <= n:
        raise ValueError("a channel of %d bins does not fit a buffer of %d" % (B, n))

    def w2(k):
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * ((np.asarray(k, dtype=np.int64) - n // 2) % n) / n)) ** 2
    g = float(np.sum(w2(np.arange(0, B // 2 + 1)))) + float(np.sum(w2(n - np.arange(1, B - B // 2))))
    if B % 2 == 0 and 2 < B < n:
        g += float(w2(n - B // 2))
    return g
