"""Squelch thresholds from a calibration pass (no reference counterpart).

``Tuner.levels()`` gives every channel's mean power of one buffer; most channels of a band monitor are empty, so the
median power density over the channels is the noise floor.  A threshold a fixed number of dB above it, scaled by each
channel's bandwidth, is what ``Tuner.set_squelch`` gates every later buffer with: calibrate occasionally, gate every
buffer.  Host numpy only; under sharding every rank calls it on its own range and supplies its own thresholds.
(A receiver with IQ imbalance puts the image of every strong station into the mirror channel and opens it: see
``Tuner.set_iq_balance`` and ``radiocore.tools.iq.balance_from``, the same recipe for the balance -- calibrate first.)
"""

import numpy as np

__all__ = ["threshold_over_floor"]


def threshold_over_floor(levels, bandwidths, db):
    """float32 [C] thresholds in the units of ``levels``: floor density = median(levels / bandwidths) (power per bin of
    bandwidth), threshold[c] = density * bandwidths[c] * 10 ** (db / 10).  bandwidths: one per channel, or a scalar."""
    levels = np.asarray(levels, dtype=np.float64)
    bandwidths = np.broadcast_to(np.asarray(bandwidths, dtype=np.float64), levels.shape)
    if levels.ndim != 1 or levels.size == 0:
        raise ValueError("levels must be a non-empty vector, one per channel")
    if not np.all(bandwidths > 0):
        raise ValueError("bandwidths must be positive")
    density = float(np.median(levels / bandwidths))
    return (density * bandwidths * 10.0 ** (float(db) / 10.0)).astype(np.float32)
