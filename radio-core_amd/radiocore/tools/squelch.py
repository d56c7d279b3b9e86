"""Squelch thresholds from a calibration pass (no reference counterpart).

``Tuner.levels()`` gives every channel's mean power of one buffer; most channels of a band monitor are empty, so the
median power density over the channels is the noise floor.  A threshold a fixed number of dB above it, scaled by each
channel's bandwidth, is what ``Tuner.set_squelch`` gates every later buffer with: calibrate occasionally, gate every
buffer.  Host numpy only; under sharding every rank calls it on its own range and supplies its own thresholds.
(A receiver with IQ imbalance puts the image of every strong station into the mirror channel and opens it: see
``Tuner.set_iq_balance`` and ``radiocore.tools.iq.balance_from``, the same recipe for the balance -- calibrate first.)
"""

import numpy as np

__all__ = ["threshold_over_floor"]          # (segments: by its module, radiocore.tools.squelch.segments)


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


def segments(frame_mask, A):
    """What a publisher sends of a buffer gated by a ``FrameGate``: ``[(channel, start_sample, stop_sample)]``, the runs of
    consecutive open frames of ``frame_mask`` (bool [C, F], ``Tuner.frame_mask()``) in audio samples of a row of ``A``
    (half-open, channel by channel, ascending).  The fade-out of a channel that closes lies in the first closed frame; a
    publisher that wants it sends ``min(stop_sample + ramp, A)``."""
    m = np.asarray(frame_mask, dtype=bool)
    if m.ndim != 2 or m.shape[1] < 1:
        raise ValueError("frame_mask is [channels, frames]")
    F = m.shape[1]
    if int(A) < 1 or int(A) % F:
        raise ValueError("%d frames do not divide a row of %d samples" % (F, int(A)))
    La = int(A) // F
    edges = np.diff(np.pad(m.astype(np.int8), ((0, 0), (1, 1))), axis=1)         # +1 where a run starts, -1 behind its end
    out = []
    for c in range(m.shape[0]):
        starts, stops = np.flatnonzero(edges[c] == 1), np.flatnonzero(edges[c] == -1)
        out.extend((c, int(a) * La, int(b) * La) for a, b in zip(starts, stops))
    return out
