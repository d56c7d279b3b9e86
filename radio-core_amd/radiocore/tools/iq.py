"""Raw integer IQ as receivers deliver it (include/rcfm.h, RCFM_IQ_*; no reference counterpart: the reference takes
complex64 only): interleaved I, Q, full scale 1.0 -- int16 (Airspy, the USRP wire format, most files), int8 (HackRF),
uint8 (RTL-SDR, centre 127.5).  ``Tuner.load_raw`` takes such a buffer as it is; ``to_complex64`` is the conversion alone,
for ``Decimate`` / ``WBFM.run`` or code of the caller's own.  Both give the same float32 values, each exactly the integer
times its power of two.
"""

import ctypes

import numpy as np

from radiocore._internal import hip

__all__ = ["to_complex64", "FORMATS"]

FORMATS = {np.dtype("int16"): hip.RCFM_IQ_CS16, np.dtype("int8"): hip.RCFM_IQ_CS8, np.dtype("uint8"): hip.RCFM_IQ_CU8}


def device_pairs(samples):
    """(flat contiguous device tensor of 2 N integers, RCFM_IQ_* format, N) of a numpy array or torch tensor shaped
    [N, 2] or [2 N]; ValueError for another dtype or shape, or an odd element count."""
    t = hip.torch()
    if isinstance(samples, t.Tensor):
        dt = {t.int16: np.dtype("int16"), t.int8: np.dtype("int8"), t.uint8: np.dtype("uint8")}.get(samples.dtype)
    else:
        samples = np.asarray(samples)
        dt = samples.dtype
    fmt = FORMATS.get(dt)
    if fmt is None:
        raise ValueError("raw IQ is int16, int8 or uint8, not %s" % (samples.dtype,))
    shape = tuple(samples.shape)
    if not (len(shape) == 1 or (len(shape) == 2 and shape[1] == 2)):
        raise ValueError("raw IQ is shaped [N, 2] or [2 N], not %s" % (list(shape),))
    if len(shape) == 1 and shape[0] % 2:
        raise ValueError("raw IQ holds I, Q pairs: an odd element count (%d)" % shape[0])
    x = hip.to_device(samples).reshape(-1)
    return x, fmt, int(x.shape[0]) // 2


def to_complex64(raw):
    """complex64 [N] device tensor of the raw buffer `raw` ([N, 2] or [2 N] int16 / int8 / uint8, host or device):
    rcfm_iq_convert on the current stream."""
    x, fmt, n = device_pairs(raw)
    out = hip.empty((n,), hip.torch().complex64)
    hip.check(hip.lib().rcfm_iq_convert(fmt, ctypes.c_size_t(n), hip.ptr(x), hip.ptr(out), hip.stream()))
    return out
