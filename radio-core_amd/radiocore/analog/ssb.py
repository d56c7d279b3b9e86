"""USB / LSB: single-sideband demodulators (no reference counterpart; include/rcfm.h, RCFM_USB / RCFM_LSB)."""

from radiocore._internal import hip
from radiocore.analog._demod import Demodulator

__all__ = ["USB", "LSB"]


class USB(Demodulator):
    """Upper sideband: Re(ifft(H fft(x))) with H = 2 on bins 1 .. (B-1)//2 -> Decimate -> RCFM_SSB_LEVEL / RMS of the
    buffer -> clip +-0.999.  The channel centre is the suppressed carrier.

    Same constructor as FM / MFM / AM; `deemphasis` is accepted and unused, and no state is carried from buffer to
    buffer.  A silent channel (RMS not positive) gives zeros.  Output: float32 (output_size, 1).  Inside a Tuner
    (`run_all` / `run_each`) the audio comes straight from the loaded wideband spectrum.

    ``agc=radiocore.AGC(...)``: a peak follower carried from buffer to buffer replaces the buffer's RMS
    (``e = max(|v|, lambda e)``, audio ``level v / max(e, floor)``): a pause no longer raises the gain of its buffer, and
    the gain does not step at buffer boundaries; ``agc_state()`` reads the follower."""

    _KIND = hip.RCFM_USB
    _CHANNELS = 1
    _AGC_LEVEL = hip.RCFM_SSB_LEVEL

    def __init__(self, input_size, output_size, deemphasis=75e-6, cuda=False, batch=1, chunk=0, agc=None):
        super().__init__(input_size, output_size, deemphasis, cuda, batch, chunk)
        self._set_agc(agc)

    def _shape(self, audio):
        return audio[0] if self._batch == 1 else audio


class LSB(USB):
    """Lower sideband: as USB with the bins below the channel centre, mirrored (H_lsb[k] = H_usb[(B - k) mod B])."""

    _KIND = hip.RCFM_LSB
