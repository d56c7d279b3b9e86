"""FrameGate: a squelch that decides per frame of the buffer, with hysteresis, hang time and look-ahead, carried from buffer
to buffer (rcfm_gate_*, include/rcfm.h; no reference counterpart).  ``Tuner.set_gate`` runs one in the level squelch's
place; ``radiocore.tools.squelch.segments`` turns its frame mask into the runs of samples a publisher sends."""

import ctypes

import numpy as np

from radiocore._internal import hip

__all__ = ["FrameGate"]


class FrameGate:
    """``FrameGate(frames=50, hang=0.25, lead=1, ramp=0.005)``: every one-second buffer is cut into ``frames`` frames (20 ms
    each by default).  A channel opens with the first frame whose power reaches its ``open`` threshold, stays open while
    the power holds its ``close`` threshold and for ``hang`` seconds after it last did, and opens ``lead`` frames early so
    that an onset is not clipped (the frames are all there when the gate decides).  The audio fades in and out over
    ``ramp`` seconds, a raised cosine.  Buffers are one second long, so ``hang`` becomes ``round(hang * frames)`` frames and
    ``ramp`` becomes ``round(ramp * A)`` samples of audio at A samples per buffer, at most one frame."""

    def __init__(self, frames=50, hang=0.25, lead=1, ramp=0.005):
        if int(frames) != frames or not 1 <= int(frames) <= hip.RCFM_GATE_MAX_FRAMES:
            raise ValueError("frames: an integer from 1 to %d, not %r" % (hip.RCFM_GATE_MAX_FRAMES, frames))
        if int(lead) != lead or int(lead) < 0:
            raise ValueError("lead: a whole number of frames, at least 0, not %r" % (lead,))
        for name, v in (("hang", hang), ("ramp", ramp)):
            if not np.isfinite(float(v)) or float(v) < 0.0:
                raise ValueError("%s: seconds, finite and at least 0, not %r" % (name, v))
        self.frames = int(frames)
        self.hang = float(hang)
        self.lead = int(lead)
        self.ramp = float(ramp)

    @property
    def hang_frames(self):
        return int(round(self.hang * self.frames))

    def fits(self, n):
        """ValueError unless the gate's frames divide rows of n samples."""
        if int(n) % self.frames != 0:
            raise ValueError("a gate of %d frames does not divide rows of %d samples" % (self.frames, int(n)))

    def ramp_samples(self, A):
        """R for audio of A samples per buffer: ``round(ramp * A)``, at most one frame."""
        self.fits(A)
        return min(int(round(self.ramp * int(A))), int(A) // self.frames)

    def ramp_array(self, A):
        """float32 [R]: the rising edge's gains, ``0.5 - 0.5 cos(pi (i + 1) / (R + 1))`` in float64, rounded once."""
        R = self.ramp_samples(A)
        return (0.5 - 0.5 * np.cos(np.pi * (np.arange(R, dtype=np.float64) + 1.0) / (R + 1.0))).astype(np.float32)

    def _create(self, C, A):
        """A new librcfm handle (every channel closed) for C channels with audio of A samples per buffer."""
        r = np.ascontiguousarray(self.ramp_array(A))
        out = ctypes.c_void_p()
        lib = hip.lib()
        hip.check(lib.rcfm_gate_create(int(C), self.hang_frames, self.lead,
                                       r.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if r.shape[0] else None,
                                       int(r.shape[0]), ctypes.byref(out)))
        return hip.Handle(out, lib.rcfm_gate_destroy)
