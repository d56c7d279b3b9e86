"""ToneBank: the power of the audio at a set of tone frequencies, per channel and time frame (rcfm_tone_bank_*,
include/rcfm.h; no reference counterpart).  ``Tuner.set_tones`` runs one behind the demodulators; ``radiocore.tools.tones``
holds the CTCSS and SELCAL tables and the host side of the detection."""

import ctypes

import numpy as np

from radiocore._internal import hip

__all__ = ["ToneBank"]


class ToneBank:
    """``ToneBank(freqs_hz, frame=None, window="hann")``: K tone frequencies in Hz (1 .. 64), a frame length in audio
    samples (None: the whole row, one frame per buffer) and a window -- ``"hann"`` (periodic), ``"rect"`` or an array of
    ``frame`` values.  Buffers are one second long, so audio of A samples puts the tone f at f / A cycles per sample; the
    device handle is made on first use per audio length and kept."""

    def __init__(self, freqs_hz, frame=None, window="hann"):
        f = np.atleast_1d(np.asarray(freqs_hz, dtype=np.float64))
        if f.ndim != 1 or not 1 <= f.shape[0] <= hip.RCFM_TONE_MAX_K:
            raise ValueError("a tone bank holds 1 .. %d frequencies" % hip.RCFM_TONE_MAX_K)
        if not np.all(np.isfinite(f)) or np.any(f < 0):
            raise ValueError("tone frequencies are finite and not negative")
        if frame is not None and int(frame) < 1:
            raise ValueError("frame is at least one sample")
        if isinstance(window, str):
            if window not in ("hann", "rect"):
                raise ValueError('window: "hann", "rect" or an array, not %r' % (window,))
        else:
            window = np.ascontiguousarray(window, dtype=np.float32)
            if window.ndim != 1 or (frame is not None and window.shape[0] != int(frame)):
                raise ValueError("a window array has one value per sample of the frame")
        self.freqs = f
        self.frame = None if frame is None else int(frame)
        self.window = window
        self._handles = {}          # audio length A -> librcfm handle

    def __len__(self):
        return int(self.freqs.shape[0])

    def index(self, tone):
        """The index of a tone: an integer is taken as the index itself (-1: none), anything else as a frequency in Hz
        that must be one of the bank's."""
        if tone is None:
            return -1
        if isinstance(tone, (int, np.integer)):
            k = int(tone)
            if not -1 <= k < len(self):
                raise ValueError("tone index %d outside -1 .. %d" % (k, len(self) - 1))
            return k
        hit = np.flatnonzero(np.isclose(self.freqs, float(tone), rtol=0.0, atol=1e-6))
        if hit.size == 0:
            raise ValueError("%r Hz is not a tone of this bank" % (tone,))
        return int(hit[0])

    def frame_length(self, A):
        return int(A) if self.frame is None else self.frame

    def window_array(self, L):
        """float32 [L] of the window, or None for "rect"."""
        if isinstance(self.window, str):
            if self.window == "rect":
                return None
            return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L, dtype=np.float64) / L)).astype(np.float32)
        if self.window.shape[0] != L:
            raise ValueError("the window has %d values, the frame %d samples" % (self.window.shape[0], L))
        return self.window

    def _handle(self, A):
        A = int(A)
        h = self._handles.get(A)
        if h is None:
            L = self.frame_length(A)
            if L > A:
                raise ValueError("input_sig size and input_size mismatch: a frame of %d samples, audio of %d" % (L, A))
            nu = np.ascontiguousarray(self.freqs / float(A))
            if np.any(nu > 0.5):
                raise ValueError("a tone lies above half the audio rate (%d Hz)" % (A // 2))
            w = self.window_array(L)
            out = ctypes.c_void_p()
            lib = hip.lib()
            hip.check(lib.rcfm_tone_bank_create(len(self), nu.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), L,
                                                w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if w is not None else None,
                                                ctypes.byref(out)))
            h = self._handles[A] = hip.Handle(out, lib.rcfm_tone_bank_destroy)
        return h.value

    def run(self, audio, step=1, offset=0, energy=True):
        """Device tensors ``(P [count, F, K], E [count, F])`` of a device tensor ``audio`` [count, A] (step = 1) or
        [count, A, 2] (step = 2, ``offset`` picks the side), on the current stream, unsynchronised.  energy=False: E is None."""
        t = hip.torch()
        count, A = int(audio.shape[0]), int(audio.shape[1])
        if audio.dtype != t.float32 or not audio.is_contiguous() or audio.numel() != count * A * int(step):
            raise ValueError("audio is a contiguous float32 tensor [count, A] or [count, A, step]")
        handle = self._handle(A)
        F = A // self.frame_length(A)
        P = hip.empty((count, F, len(self)), t.float32)
        E = hip.empty((count, F), t.float32) if energy else None
        hip.check(hip.lib().rcfm_tone_bank_run(handle, hip.ptr(audio), count, A, int(step), int(offset), hip.ptr(P),
                                               hip.ptr(E) if energy else None, hip.stream()))
        return P, E
