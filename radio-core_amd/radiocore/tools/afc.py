"""Frequency corrections from a carrier pass (no reference counterpart).

``Tuner.carriers()`` says where inside its channel each station sits; ``Tuner.retune`` moves the channels there.  This
is the step between the two: which channels to move, and how far.  A channel whose strongest bin is below
``gate_power`` holds no station worth following and stays where it is; the others move by the measured offset, at most
``max_step`` bins per pass.  Calibrate occasionally, as with ``squelch.threshold_over_floor``: no hysteresis and no loop
filter.  Host numpy only; under sharding every rank calls it on its own range.
"""

import numpy as np

__all__ = ["corrections"]


def corrections(peak_bin, peak_power, centroid, gate_power, max_step, use="peak"):
    """int64 [C] offsets for ``Tuner.retune``: 0 where ``peak_power < gate_power`` (or is NaN), else ``peak_bin``
    (use="peak") or the rounded ``centroid`` (use="centroid"), clipped to +-``max_step``.  gate_power: a scalar or one
    per channel, in the units of ``peak_power``."""
    if use not in ("peak", "centroid"):
        raise ValueError("use: 'peak' or 'centroid'")
    if max_step < 0:
        raise ValueError("max_step must be >= 0")
    peak_power = np.asarray(peak_power, dtype=np.float64)
    if peak_power.ndim != 1:
        raise ValueError("one value per channel")
    offset = np.asarray(peak_bin if use == "peak" else centroid, dtype=np.float64)
    if offset.shape != peak_power.shape:
        raise ValueError("peak_bin, peak_power and centroid must have one shape")
    gate_power = np.broadcast_to(np.asarray(gate_power, dtype=np.float64), peak_power.shape)
    with np.errstate(invalid="ignore"):
        on = (peak_power >= gate_power) & np.isfinite(offset)
    step = np.clip(np.rint(np.where(on, offset, 0.0)), -int(max_step), int(max_step))
    return step.astype(np.int64)
