"""Audio egress: the way out of the device, the counterpart of ``Tuner.load_raw`` + ``Feeder`` (no reference counterpart:
the reference's loop publishes float32 arrays it already holds on the host, examples/multi_fm_server.py:103-106).

``PCM`` says what a publisher wants -- int16 samples at a gain, or float32 unchanged -- and ``Tuner.run_all_packed(pcm)``
packs the audio of the channels the squelch left open densely in that form on the device (librcfm's rcfm_audio_pack).
``Drain`` keeps `depth` device slots with page-locked host mirrors and two copy streams (rcfm_drain_*), so the audio of
buffer i crosses PCIe under the kernels of buffer i+1, and only the open rows cross:

    pcm, drain = PCM("int16"), Drain(len(tuner.channels()), (A, ch), "int16", depth=2)
    for i in range(k):
        tuner.load(x[i])
        tuner.run_all_packed(pcm, drain=drain)        # kernels + pack of buffer i, queued
        if i > 0:
            with drain.next() as (index, audio):      # buffer i-1: waits for its header, copies its open rows only
                publish(wire.frames_packed(tuner.channels(), index, audio))
    with drain.next() as (index, audio):
        publish(wire.frames_packed(tuner.channels(), index, audio))
"""

import ctypes
import math
from contextlib import contextmanager

import numpy as np

from radiocore._internal import Injector, hip

__all__ = ["PCM", "Drain"]

_FORMATS = {np.dtype("int16"): hip.RCFM_PCM_S16, np.dtype("float32"): hip.RCFM_PCM_F32}


def _pcm_dtype(dtype):
    try:
        dt = np.dtype(dtype)
    except TypeError:
        dt = None
    if dt not in _FORMATS:
        raise ValueError("PCM dtype is 'int16' or 'float32', not %r" % (dtype,))
    return dt


class PCM:
    """Sample format of packed audio (include/rcfm.h, RCFM_PCM_*).  dtype="int16": round(x * gain) to nearest even, clamped
    to +-32767, NaN -> 0; gain finite and in (0, 2**24].  dtype="float32": the samples unchanged (compaction only; gain is
    ignored).  A settings object: it needs no device."""

    def __init__(self, dtype="int16", gain=32767.0):
        self.dtype = _pcm_dtype(dtype)
        self.format = _FORMATS[self.dtype]
        try:
            with np.errstate(over="ignore"):
                gain = float(np.float32(gain))            # the float32 the ABI receives (an overflow is refused below)
        except (TypeError, ValueError):
            raise ValueError("PCM gain must be a number")
        if self.format == hip.RCFM_PCM_S16 and not (math.isfinite(gain) and 0.0 < gain <= 2.0 ** 24):
            raise ValueError("PCM gain must be finite and in (0, 2**24]")
        self.gain = gain

    def __repr__(self):
        return "PCM(dtype=%r, gain=%r)" % (self.dtype.name, self.gain)


class Drain(Injector):
    """`depth` slots for the packed audio of up to `rows` channels of `row_shape` samples of `dtype` each: device memory
    the pack kernel fills and a page-locked host mirror, drained on two copy streams behind the compute stream."""

    def __init__(self, rows, row_shape, dtype="int16", depth=2):
        self._handle = None
        self._dtype = _pcm_dtype(dtype)
        self._rows = int(rows)
        self._row_shape = tuple(int(v) for v in (row_shape if np.ndim(row_shape) else (row_shape,)))
        self._row = int(np.prod(self._row_shape, dtype=np.int64)) if self._row_shape else 0
        if self._row < 1 or any(v < 1 for v in self._row_shape):
            raise ValueError("Drain row_shape must have at least one sample")
        super().__init__(True)
        h = ctypes.c_void_p()
        hip.check(self._lib.rcfm_drain_create(self._row * self._dtype.itemsize, self._rows, int(depth), ctypes.byref(h)))
        self._handle = hip.Handle(h, self._lib.rcfm_drain_destroy)
        self._depth = int(depth)

    @property
    def depth(self):
        return self._depth

    @property
    def rows(self):
        return self._rows

    @property
    def row_shape(self):
        return self._row_shape

    @property
    def dtype(self):
        return self._dtype

    def _begin(self):
        """(packed, index, n_open) device pointers of the next free slot; RuntimeError when every slot is in flight."""
        p, ix, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        hip.check(self._lib.rcfm_drain_begin(self._handle.value, ctypes.byref(p), ctypes.byref(ix), ctypes.byref(n)))
        return p, ix, n

    def _submit(self):
        """The pack of the slot `_begin` gave out is queued on the current stream: queue its header's copy."""
        hip.check(self._lib.rcfm_drain_submit(self._handle.value, hip.stream()))

    @contextmanager
    def next(self):
        """The oldest submitted buffer as ``(index int32 [n_open], audio [n_open, *row_shape])``: numpy views of the
        page-locked slot, valid inside the block (copy what must outlive it); the slot is free again on exit.  Waits
        for that buffer's header, then copies exactly its open rows.  RuntimeError with nothing submitted."""
        n, ix, rows = ctypes.c_int(), ctypes.c_void_p(), ctypes.c_void_p()
        hip.check(self._lib.rcfm_drain_acquire(self._handle.value, ctypes.byref(n), ctypes.byref(ix), ctypes.byref(rows)))
        k = int(n.value)
        try:
            if k == 0:
                yield np.zeros(0, np.int32), np.zeros((0,) + self._row_shape, self._dtype)
            else:
                index = np.frombuffer((ctypes.c_char * (4 * k)).from_address(ix.value), dtype=np.int32)
                audio = np.frombuffer((ctypes.c_char * (k * self._row * self._dtype.itemsize)).from_address(rows.value),
                                      dtype=self._dtype).reshape((k,) + self._row_shape)
                yield index, audio
        finally:
            hip.check(self._lib.rcfm_drain_release(self._handle.value))

    def close(self):
        """Destroy the drain: waits for both copy streams, then frees the slots.  Views handed out by ``next`` die with it."""
        if self._handle is not None and self._handle.value:
            status = self._lib.rcfm_drain_destroy(self._handle.value)
            self._handle.value = None
            hip.check(status)

    def __del__(self):
        try:
            self.close()
        except Exception:               # interpreter shutdown
            pass
