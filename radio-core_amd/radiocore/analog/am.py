"""AM: envelope detector with carrier normalisation (no reference counterpart; include/rcfm.h, RCFM_AM)."""

from radiocore._internal import hip
from radiocore.analog._demod import Demodulator

__all__ = ["AM"]


class AM(Demodulator):
    """|x| -> Decimate -> divide by the buffer's mean (the carrier) -> minus 1 -> clip +-0.999.

    Same constructor as FM / MFM; `deemphasis` is accepted and unused, and AM carries no state from buffer to
    buffer.  A channel whose carrier is not positive (all zeros) gives zeros.  Output: float32 (output_size, 1).

    ``agc=radiocore.AGC(...)``: the carrier is followed from buffer to buffer instead (``c += alpha (v - c)``, audio
    ``level (v - c) / max(c, floor)``), so the gain no longer steps at buffer boundaries; ``agc_state()`` reads it."""

    _KIND = hip.RCFM_AM
    _CHANNELS = 1
    _AGC_LEVEL = 1.0

    def __init__(self, input_size, output_size, deemphasis=75e-6, cuda=False, batch=1, chunk=0, agc=None):
        super().__init__(input_size, output_size, deemphasis, cuda, batch, chunk)
        self._set_agc(agc)

    def _shape(self, audio):
        return audio[0] if self._batch == 1 else audio
