"""AGC: a gain carried from buffer to buffer for AM, USB and LSB (no reference counterpart; include/rcfm.h, rcfm_demod_set_agc)."""

import math

__all__ = ["AGC"]


class AGC:
    """What ``AM(..., agc=AGC(...))``, ``USB`` and ``LSB`` take instead of their per-buffer normalisation.

    decay   seconds in which the follower falls to 1/e: the peak follower of USB / LSB (``e = max(|v|, lambda e)``) or the
            carrier follower of AM (``c += alpha (v - c)``); ``decay * output_size`` samples
    level   what the followed quantity is scaled to: a single tone's peak (USB / LSB, default 0.25) or the audio of a
            fully modulated carrier (AM, default 1.0)
    floor   the follower never divides by less: the gain is at most ``level / floor`` (0: unbounded, an empty channel
            comes out at full scale)

    The follower's value is carried from buffer to buffer, one float per channel (``Demodulator.agc_state()``; -1 = no
    history yet).  Two AGC objects with equal settings are equal: channels of one setting run as one batch in a Tuner."""

    def __init__(self, decay=0.3, level=None, floor=0.0):
        self.decay = float(decay)
        self.level = None if level is None else float(level)
        self.floor = float(floor)
        # what rcfm_demod_set_agc would refuse is refused here
        if not (math.isfinite(self.decay) and self.decay > 0.0):
            raise ValueError("AGC decay must be finite and > 0")
        if self.level is not None and not (math.isfinite(self.level) and self.level > 0.0):
            raise ValueError("AGC level must be finite and > 0")
        if not (math.isfinite(self.floor) and self.floor >= 0.0):
            raise ValueError("AGC floor must be finite and >= 0")

    def _settings(self, output_size, default_level):
        """(decay_samples, level, floor) as rcfm_demod_set_agc takes them: the Tuner's key for this setting."""
        return (self.decay * output_size, default_level if self.level is None else self.level, self.floor)

    def __eq__(self, other):
        return isinstance(other, AGC) and (self.decay, self.level, self.floor) == (other.decay, other.level, other.floor)

    def __hash__(self):
        return hash((self.decay, self.level, self.floor))

    def __repr__(self):
        return "AGC(decay=%r, level=%r, floor=%r)" % (self.decay, self.level, self.floor)
