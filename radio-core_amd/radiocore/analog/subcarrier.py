"""Subcarrier tap: the complex baseband of the FM multiplex around one subcarrier (no reference counterpart;
include/rcfm.h, rcfm_subcarrier_*)."""

import ctypes

import numpy as np

from radiocore._internal import Injector, hip

__all__ = ["Subcarrier"]

MAX_TAPS = 4095


def check_arguments(input_size, output_size, frequency, taps, batch=1):
    """What rcfm_subcarrier_create would refuse, as ValueError; returns (B, R, f, float32 taps)."""
    B, R, batch = int(input_size), int(output_size), int(batch)
    if frequency != int(frequency):
        raise ValueError("the subcarrier frequency is a whole number of Hz")
    f = int(frequency)
    if batch < 1 or B < 2 or R < 1:
        raise ValueError("bad subcarrier tap size")
    if B % R != 0:
        raise ValueError("the output length must divide the input length")
    if abs(f) > B // 2:
        raise ValueError("subcarrier frequency beyond half the sample rate")
    h = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
    if len(h) < 1 or len(h) > MAX_TAPS or len(h) % 2 == 0:
        raise ValueError("the number of taps must be odd, 1 .. %d" % MAX_TAPS)
    if not np.all(np.isfinite(h)):
        raise ValueError("a tap is not finite")
    return B, R, f, h


class Subcarrier(Injector):
    """Mixes the discriminator output of `input_size` channel samples down by `frequency` Hz (a whole number, either
    sign, at most input_size / 2), low-pass filters it with the real `taps` (an odd number, at most 4095) and keeps
    every (input_size / output_size)-th sample: complex64 (output_size,), or (batch, output_size) from a
    [batch, input_size] array for batch > 1.  A subcarrier at `frequency` with deviation D Hz and phase p comes out as
    (D / input_size) sum(taps) exp(1j p).  ``radiocore.tools.rds.taps`` designs the low-pass RDS needs; a Tuner runs a
    tap over its channels with ``Tuner.subcarrier(tap)``."""

    def __init__(self, input_size, output_size, frequency, taps, cuda=False, batch=1, chunk=0):
        self._cuda = cuda
        self._batch = int(batch)
        self._chunk = int(chunk)
        super().__init__(cuda)
        self._input_size, self._output_size, self._frequency, self._taps = \
            check_arguments(input_size, output_size, frequency, taps, batch)
        self._h = None      # created on first use, like the demodulators' handles

    def _key(self):
        return self._input_size, self._output_size, self._frequency, self._taps.tobytes()

    def _create(self, channels, chunk):
        h = ctypes.c_void_p()
        _, fp = hip.float_array(self._taps)
        hip.check(self._lib.rcfm_subcarrier_create(int(channels), self._input_size, self._output_size, self._frequency, fp,
                                                   len(self._taps), int(chunk), ctypes.byref(h)))
        return hip.Handle(h, self._lib.rcfm_subcarrier_destroy)

    @property
    def _handle(self):
        if self._h is None:
            self._h = self._create(self._batch, self._chunk)
        return self._h

    def run(self, input_sig, numpy_output=True):
        t = self._torch
        if self._batch == 1 and len(input_sig) != self._input_size:
            raise ValueError("input_sig size and input_size mismatch")
        x = hip.to_device(input_sig, t.complex64)
        if self._batch > 1 and tuple(x.shape) != (self._batch, self._input_size):
            raise ValueError("input_sig size and input_size mismatch")
        y = hip.empty((self._batch, self._output_size), t.complex64)
        hip.check(self._lib.rcfm_subcarrier_run(self._handle.value, self._batch, hip.ptr(x), hip.ptr(y), hip.stream()))
        y = y[0] if self._batch == 1 else y
        return self._result(y, self._cuda and not numpy_output)
