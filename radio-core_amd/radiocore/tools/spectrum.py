"""The geometry of ``Tuner.power_spectrum`` and what a scan reads from it (no reference counterpart).

``Tuner.power_spectrum(cells, f_lo, f_hi)`` bins the loaded wideband spectrum: signed bin ``s`` is ``s`` Hz from the
input frequency (buffers are one second long), a span ``[s0, s0 + L)`` of them is cut into ``cells`` cells, and cell
``m`` covers span positions ``[m * L // cells, (m + 1) * L // cells)`` -- the rule of include/rcfm.h.  The helpers here say
where the span and the cells lie and pick the occupied runs of cells out of the result.  Host numpy only.
"""

import numpy as np

__all__ = ["span_bins", "cell_edges", "cell_frequencies", "occupied"]


def span_bins(input_frequency, n, f_lo=None, f_hi=None):
    """(s0, L): the signed bins of [f_lo, f_hi) Hz in the spectrum of an n-sample, one-second buffer centred on
    input_frequency -- s0 = round(f_lo - input_frequency), s0 + L = round(f_hi - input_frequency), half-open.  None is
    the band's own end: the signed bins run from -(n // 2) to n - n // 2.  ValueError for an empty span or one that
    leaves the band."""
    n = int(n)
    if n < 1:
        raise ValueError("the buffer has no samples")
    lo, hi = -(n // 2), n - n // 2
    s0 = lo if f_lo is None else int(round(float(f_lo) - float(input_frequency)))
    s1 = hi if f_hi is None else int(round(float(f_hi) - float(input_frequency)))
    if s1 <= s0:
        raise ValueError("empty span: f_hi must lie above f_lo")
    if s0 < lo or s1 > hi:
        raise ValueError("span [%d, %d) Hz from the input frequency leaves the band [%d, %d)" % (s0, s1, lo, hi))
    return s0, s1 - s0


def cell_edges(L, cells):
    """int64 [cells + 1]: cell m covers span positions [edges[m], edges[m + 1]), edges[m] = m * L // cells (64-bit)."""
    L, cells = int(L), int(cells)
    if L < 1 or cells < 1 or cells > L:
        raise ValueError("a span of %d bins takes 1 .. %d cells, not %d" % (L, max(L, 0), cells))
    return np.arange(cells + 1, dtype=np.int64) * np.int64(L) // np.int64(cells)


def cell_frequencies(input_frequency, s0, L, cells):
    """float64 [cells]: the centre frequency of each cell in Hz (the mean of the frequencies of its bins)."""
    e = cell_edges(L, cells)
    return float(input_frequency) + int(s0) + 0.5 * (e[:-1] + e[1:] - 1)


def occupied(power, db, min_cells=1, lengths=None, floor=None):
    """The occupied runs of a binned power spectrum: [(first_cell, last_cell, strongest_cell)], inclusive.

    The floor is the median power density, median(power / lengths) (lengths: bins per cell, one per cell or a scalar;
    None: equal cells); a cell is kept when its density is at least ``db`` dB above it, and every contiguous run of at
    least ``min_cells`` kept cells is reported with the cell of its highest power.  ``floor``: one value per cell in the
    units of ``power`` (``Tuner.floor()``) takes the global median's place -- a cell is kept when its power is at least
    ``db`` dB above its own floor; a cell whose floor is NaN is not kept."""
    power = np.asarray(power, dtype=np.float64)
    if power.ndim != 1 or power.size == 0:
        raise ValueError("power must be a non-empty vector, one value per cell")
    lengths = np.broadcast_to(np.asarray(1.0 if lengths is None else lengths, dtype=np.float64), power.shape)
    if not np.all(lengths > 0):
        raise ValueError("cell lengths must be positive")
    density = power / lengths
    if floor is None:
        keep = density >= float(np.median(density)) * 10.0 ** (float(db) / 10.0)
    else:
        floor = np.asarray(floor, dtype=np.float64)
        if floor.shape != power.shape:
            raise ValueError("floor: one value per cell (%d), not %s" % (power.size, floor.shape))
        with np.errstate(invalid="ignore"):
            keep = density >= floor / lengths * 10.0 ** (float(db) / 10.0)
    # run boundaries: where `keep` changes, with a closed cell assumed beyond both ends
    change = np.flatnonzero(np.diff(np.concatenate(([False], keep, [False])).astype(np.int8)))
    runs = []
    for a, b in zip(change[0::2], change[1::2]):          # cells [a, b)
        if b - a >= int(min_cells):
            runs.append((int(a), int(b) - 1, int(a + np.argmax(power[a:b]))))
    return runs
