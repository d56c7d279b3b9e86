"""NoiseBlanker: impulse noise removed from the wideband buffer, ahead of the Tuner's FFT (rcfm_blanker_*, include/rcfm.h,
"noise blanker"; no reference counterpart).  A pulse of a few samples -- ignition, a switching supply, an electric fence -- is
white across the band: once ``Tuner.load`` has run it sits in every channel.  The blanker finds the samples whose power
stands out over the median level of the neighbouring blocks and takes the buffer to zero around them.
``Tuner.set_blanker`` runs one ahead of every load; ``run`` is the stage alone."""

import ctypes

import numpy as np

from radiocore._internal import hip

__all__ = ["NoiseBlanker"]

_NUMPY_FORMATS = {np.dtype("complex64"): hip.RCFM_IQ_CF32, np.dtype("complex128"): hip.RCFM_IQ_CF32,
                  np.dtype("int16"): hip.RCFM_IQ_CS16, np.dtype("int8"): hip.RCFM_IQ_CS8, np.dtype("uint8"): hip.RCFM_IQ_CU8}
_SAMPLE_BYTES = {hip.RCFM_IQ_CF32: 8, hip.RCFM_IQ_CS16: 4, hip.RCFM_IQ_CS8: 2, hip.RCFM_IQ_CU8: 2}


class NoiseBlanker:
    """``NoiseBlanker(threshold_db=12.0, hold=2e-6, ramp=1e-6, block=4096, span=4, absolute=None)``

    A sample is a hit when its power exceeds ``threshold_db`` over the lower median of the mean powers of the ``2 span + 1``
    blocks of ``block`` samples around it (``absolute``: a fixed power threshold instead, full scale 1.0, and no level pass).
    Around a hit the buffer is zero for ``hold`` seconds each way and comes back over ``ramp`` seconds along a raised cosine
    built here in float64, ``0.5 (1 - cos(pi (j + 1) / (R + 1)))``.  Buffers are one second long, so both times are
    discretised per buffer length: ``round(hold n)`` and ``round(ramp n)`` samples, together at most 1024.  One device handle
    is made per buffer length and kept.  ValueError for whatever the library would refuse, before it is called."""

    def __init__(self, threshold_db=12.0, hold=2e-6, ramp=1e-6, block=4096, span=4, absolute=None):
        threshold_db, hold, ramp = float(threshold_db), float(hold), float(ramp)
        if not np.isfinite(threshold_db):
            raise ValueError("threshold_db is finite")
        if absolute is not None:
            absolute = float(absolute)
            if not (np.isfinite(absolute) and absolute > 0.0):
                raise ValueError("an absolute threshold is a finite, positive power")
        if not (np.isfinite(hold) and hold >= 0.0 and np.isfinite(ramp) and ramp >= 0.0):
            raise ValueError("hold and ramp are times in seconds, finite and not negative")
        block, span = int(block), int(span)
        if block < hip.RCFM_BLANK_MIN_BLOCK or block > hip.RCFM_BLANK_MAX_BLOCK or block & (block - 1):
            raise ValueError("block is a power of two, %d .. %d" % (hip.RCFM_BLANK_MIN_BLOCK, hip.RCFM_BLANK_MAX_BLOCK))
        if not 0 <= span <= hip.RCFM_BLANK_MAX_SPAN:
            raise ValueError("span is 0 .. %d blocks" % hip.RCFM_BLANK_MAX_SPAN)
        self.threshold_db, self.hold, self.ramp, self.block, self.span, self.absolute = threshold_db, hold, ramp, block, span, absolute
        self.mode = hip.RCFM_BLANK_MEDIAN if absolute is None else hip.RCFM_BLANK_ABSOLUTE
        try:
            self.value = 10.0 ** (threshold_db / 10.0) if absolute is None else absolute
        except OverflowError:
            self.value = float("inf")
        if not (np.isfinite(self.value) and self.value > 0.0):
            raise ValueError("threshold_db gives no finite, positive power ratio")
        self._handles = {}          # buffer length n -> librcfm handle of run()

    def geometry(self, n):
        """(hold in samples, ramp table float32 [R]) for buffers of n samples; ValueError when they exceed 1024 samples."""
        n = int(n)
        if n < 0:
            raise ValueError("a buffer has at least 0 samples")
        H, R = int(round(self.hold * n)), int(round(self.ramp * n))
        if H + R > hip.RCFM_BLANK_MAX_GUARD:
            raise ValueError("hold + ramp are %d samples of a %d-sample buffer: at most %d" % (H + R, n, hip.RCFM_BLANK_MAX_GUARD))
        j = np.arange(R, dtype=np.float64)
        return H, (0.5 * (1.0 - np.cos(np.pi * (j + 1.0) / (R + 1.0)))).astype(np.float32)

    def _create(self, n):
        """A device handle of its own for buffers of n samples (Tuner.set_blanker keeps one per device tuner: lanes share
        the NoiseBlanker, not its scratch)."""
        H, ramp = self.geometry(n)
        if n < 1:
            raise ValueError("a blanker handle is made for buffers of at least one sample")
        out = ctypes.c_void_p()
        lib = hip.lib()
        hip.check(lib.rcfm_blanker_create(int(n), self.block, self.span, self.mode, self.value, H,
                                          ramp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if ramp.shape[0] else None,
                                          int(ramp.shape[0]), ctypes.byref(out)))
        return hip.Handle(out, lib.rcfm_blanker_destroy)

    def _handle(self, n):
        h = self._handles.get(int(n))
        if h is None:
            h = self._handles[int(n)] = self._create(int(n))
        return h.value

    @staticmethod
    def describe(x):
        """(RCFM_IQ_* format, samples) of a buffer: complex64 [n] (numpy complex128 is converted), or interleaved int16 /
        int8 / uint8 shaped [n, 2] or [2 n]; ValueError otherwise.  No device is touched."""
        if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
            x = np.asarray(x)
            fmt = _NUMPY_FORMATS.get(x.dtype)
        else:
            fmt = {"torch.complex64": hip.RCFM_IQ_CF32, "torch.int16": hip.RCFM_IQ_CS16, "torch.int8": hip.RCFM_IQ_CS8,
                   "torch.uint8": hip.RCFM_IQ_CU8}.get(str(x.dtype))
        if fmt is None:
            raise ValueError("a buffer is complex64, or interleaved int16, int8 or uint8, not %s" % (x.dtype,))
        shape = tuple(x.shape)
        if fmt == hip.RCFM_IQ_CF32:
            if len(shape) != 1:
                raise ValueError("a complex64 buffer is shaped [n], not %s" % (list(shape),))
            return fmt, int(shape[0])
        if not (len(shape) == 1 or (len(shape) == 2 and shape[1] == 2)):
            raise ValueError("raw IQ is shaped [N, 2] or [2 N], not %s" % (list(shape),))
        if len(shape) == 1 and shape[0] % 2:
            raise ValueError("raw IQ holds I, Q pairs: an odd element count (%d)" % shape[0])
        return fmt, int(shape[0]) if len(shape) == 2 else int(shape[0]) // 2

    def run(self, x, out=None, stats=False):
        """The stage alone, on the current stream: the blanked buffer, in x's format and shape -- a numpy array for a numpy
        array (it is uploaded, blanked in place on the device and copied back), a device tensor for a device tensor, which
        is left untouched unless ``out`` is x itself (in place).  ``out``: a contiguous device tensor of x's dtype and
        shape to write into.  stats=True: ``(y, (hits, blanked))``, the number of hits and of samples whose gain is below 1
        (a host synchronisation)."""
        fmt, n = self.describe(x)
        self.geometry(n)
        t = hip.torch()
        host = not isinstance(x, t.Tensor)
        src = hip.to_device(x, t.complex64 if fmt == hip.RCFM_IQ_CF32 else None)
        fresh = host or not x.is_cuda or src.data_ptr() != x.data_ptr()
        if out is None:
            dst = src if fresh else t.empty_like(src)
        else:
            if not isinstance(out, t.Tensor) or not out.is_cuda or not out.is_contiguous() or out.dtype != src.dtype or \
                    tuple(out.shape) != tuple(src.shape):
                raise ValueError("out is a contiguous device tensor of the buffer's dtype and shape")
            dst = out
        elem = _SAMPLE_BYTES[fmt]
        a, o, nbytes = src.data_ptr(), dst.data_ptr(), n * elem
        if a % elem or o % elem:
            raise ValueError("a buffer is aligned for one sample (%d bytes)" % elem)
        if a != o and a < o + nbytes and o < a + nbytes:
            raise ValueError("in and out overlap in part: they are the same buffer or disjoint")
        counts = hip.empty((2,), t.int64) if stats else None
        if n > 0:
            hip.check(hip.lib().rcfm_blanker_run(self._handle(n), fmt, n, hip.ptr(src), hip.ptr(dst),
                                                 hip.ptr(counts) if stats else None, hip.stream()))
        elif stats:
            counts.zero_()
        elif dst is not src:
            dst.copy_(src)
        y = hip.to_host(dst) if host else dst
        if stats:
            c = hip.to_host(counts)
            return y, (int(c[0]), int(c[1]))
        return y
