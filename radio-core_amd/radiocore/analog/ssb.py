"""USB / LSB: single-sideband demodulators (no reference counterpart; include/rcfm.h, RCFM_USB / RCFM_LSB)."""

from radiocore._internal import hip
from radiocore.analog._demod import Demodulator

__all__ = ["USB", "LSB"]


class USB(Demodulator):
    """Upper sideband: Re(ifft(H fft(x))) with H = 2 on bins 1 .. (B-1)//2 -> Decimate -> RCFM_SSB_LEVEL / RMS of the
    buffer -> clip +-0.999.  The channel centre is the suppressed carrier.

    Same constructor as FM / MFM / AM; `deemphasis` is accepted and unused, and no state is carried from buffer to
    buffer.  A silent channel (RMS not positive) gives zeros.  Output: float32 (output_size, 1).  Inside a Tuner
    (`run_all` / `run_each`) the audio comes straight from the loaded wideband spectrum."""

    _KIND = hip.RCFM_USB
    _CHANNELS = 1

    def _shape(self, audio):
        return audio[0] if self._batch == 1 else audio


class LSB(USB):
    """Lower sideband: as USB with the bins below the channel centre, mirrored (H_lsb[k] = H_usb[(B - k) mod B])."""

    _KIND = hip.RCFM_LSB
