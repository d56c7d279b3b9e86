"""AM: envelope detector with carrier normalisation (no reference counterpart; include/rcfm.h, RCFM_AM)."""

from radiocore._internal import hip
from radiocore.analog._demod import Demodulator

__all__ = ["AM"]


class AM(Demodulator):
    """|x| -> Decimate -> divide by the buffer's mean (the carrier) -> minus 1 -> clip +-0.999.

    Same constructor as FM / MFM; `deemphasis` is accepted and unused, and AM carries no state from buffer to
    buffer.  A channel whose carrier is not positive (all zeros) gives zeros.  Output: float32 (output_size, 1)."""

    _KIND = hip.RCFM_AM
    _CHANNELS = 1

    def _shape(self, audio):
        return audio[0] if self._batch == 1 else audio
