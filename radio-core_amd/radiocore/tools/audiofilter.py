"""AudioFilter: biquad sections on the audio of every channel, carried from buffer to buffer (rcfm_audio_filter_*,
include/rcfm.h; no reference counterpart).  A filter is described in Hz and seconds and discretised per audio rate;
``Tuner.set_audio_filter`` runs one behind the demodulators.  The Butterworth designs are written out here (analogue
prototype, band transform, bilinear transform with pre-warped corners -- what ``scipy.signal.butter`` computes), so the
package needs no scipy."""

import ctypes

import numpy as np

from radiocore._internal import hip

__all__ = ["AudioFilter"]

_MAX = hip.RCFM_SOS_MAX_SECTIONS


def _prototype(order):
    """Poles of the analogue Butterworth low-pass of corner 1 rad/s: the upper half plane's, and whether -1 is one."""
    k = np.arange(order // 2)
    return np.exp(1j * np.pi * (2.0 * k + order + 1.0) / (2.0 * order)), bool(order % 2)


def _section(zeros, poles):
    """b0 b1 b2 1 a1 a2 of up to two zeros and a conjugate pair / one or two real poles, without gain."""
    b = np.real(np.poly(zeros))
    a = np.real(np.poly(poles))
    return np.concatenate([np.pad(b, (0, 3 - b.size)), np.pad(a, (0, 3 - a.size))])


def _normalise(sos, z):
    """Unit gain at the point z of the unit circle, section by section."""
    zi = 1.0 / z
    for row in sos:
        h = (row[0] + row[1] * zi + row[2] * zi * zi) / (row[3] + row[4] * zi + row[5] * zi * zi)
        row[:3] /= abs(h)
    return sos


def _corner(f_hz, A, what):
    f = float(f_hz)
    if not np.isfinite(f) or f <= 0.0:
        raise ValueError("%s: a corner frequency is finite and positive, not %r" % (what, f_hz))
    if f >= A / 2.0:
        raise ValueError("%s: the corner %g Hz is at or above half the audio rate (%d Hz)" % (what, f, A // 2))
    return 2.0 * A * np.tan(np.pi * f / A)       # pre-warped, rad/s


def _butter(kind, corners, order, A):
    fs2 = 2.0 * A
    upper, real = _prototype(order)
    rows = []
    if kind == "bandpass":
        w1, w2 = _corner(corners[0], A, kind), _corner(corners[1], A, kind)
        bw, w0 = w2 - w1, np.sqrt(w1 * w2)
        for p in upper:                           # one prototype pole -> two band-pass poles, each with its conjugate
            h = p * bw / 2.0
            d = np.sqrt(h * h - w0 * w0)
            for s in (h + d, h - d):
                z = (fs2 + s) / (fs2 - s)
                rows.append(_section([1.0, -1.0], [z, np.conj(z)]))
        if real:
            h = -bw / 2.0
            d = np.sqrt(complex(h * h - w0 * w0))
            rows.append(_section([1.0, -1.0], [(fs2 + h + d) / (fs2 - h - d), (fs2 + h - d) / (fs2 - h + d)]))
        return _normalise(np.array(rows), np.exp(2j * np.arctan(w0 / fs2)))
    wc = _corner(corners[0], A, kind)
    zero = -1.0 if kind == "lowpass" else 1.0
    for p in upper:
        s = wc * p if kind == "lowpass" else wc / p
        z = (fs2 + s) / (fs2 - s)
        rows.append(_section([zero, zero], [z, np.conj(z)]))
    if real:
        rows.append(_section([zero], [(fs2 - wc) / (fs2 + wc)]))
    return _normalise(np.array(rows), 1.0 if kind == "lowpass" else -1.0)


def _check_sos(sos):
    """What rcfm_audio_filter_create refuses, as a ValueError before any device call."""
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= _MAX:
        raise ValueError("sos: float64 [S][6] with 1 <= S <= %d" % _MAX)
    if not np.all(np.isfinite(sos)):
        raise ValueError("sos: a coefficient is not finite")
    if np.any(sos[:, 3] != 1.0):
        raise ValueError("sos: every section's a0 is exactly 1")
    if np.any(np.abs(sos[:, 5]) >= 1.0) or np.any(np.abs(sos[:, 4]) >= 1.0 + sos[:, 5]):
        raise ValueError("sos: a section is not strictly stable (|a2| < 1 and |a1| < 1 + a2)")
    return sos


class AudioFilter:
    """S <= 8 biquad sections per channel with state that survives the buffer boundary.  Built from the constructors
    ``highpass`` / ``lowpass`` / ``bandpass`` (Butterworth, corners in Hz), ``deemphasis(tau)`` and ``sos(array, rate)``,
    concatenated with ``+``.  Buffers are one second long, so a row of A samples has the rate A: ``sections(A)`` is the
    design for it, float64 [S][6] in scipy's ``sos`` layout."""

    def __init__(self, parts=()):
        self._parts = tuple(parts)
        if not 1 <= len(self) <= _MAX:
            raise ValueError("an audio filter holds 1 .. %d sections, not %d" % (_MAX, len(self)))
        self._sections = {}         # A -> float64 [S][6]
        self._handles = {}          # (C, ch, A) -> librcfm handle of run()

    @staticmethod
    def _order(order):
        n = int(order)
        if n != order or not 1 <= n <= 2 * _MAX:
            raise ValueError("order: an integer from 1 to %d, not %r" % (2 * _MAX, order))
        return n

    @classmethod
    def highpass(cls, f_hz, order=4):
        n = cls._order(order)
        return cls([("highpass", (float(f_hz),), n, (n + 1) // 2)])

    @classmethod
    def lowpass(cls, f_hz, order=4):
        n = cls._order(order)
        return cls([("lowpass", (float(f_hz),), n, (n + 1) // 2)])

    @classmethod
    def bandpass(cls, lo_hz, hi_hz, order=4):
        """Pass band lo_hz .. hi_hz; ``order`` as scipy.signal.butter takes it: the filter has ``order`` sections."""
        n = cls._order(order)
        if not float(lo_hz) < float(hi_hz):
            raise ValueError("bandpass: lo_hz < hi_hz")
        return cls([("bandpass", (float(lo_hz), float(hi_hz)), n, n)])

    @classmethod
    def deemphasis(cls, tau):
        """One first-order section 1 / (1 + s tau), bilinear with the corner 1 / (2 pi tau) kept in place; gain 1 at DC."""
        tau = float(tau)
        if not np.isfinite(tau) or tau <= 0.0:
            raise ValueError("deemphasis: tau is finite and positive")
        return cls([("deemphasis", (tau,), 1, 1)])

    @classmethod
    def sos(cls, array, rate):
        """A digital design as it stands, valid for rows of exactly ``rate`` samples."""
        a = _check_sos(np.array(array, dtype=np.float64))
        if int(rate) != rate or int(rate) < 1:
            raise ValueError("sos: rate is a positive integer")
        return cls([("sos", (a, int(rate)), 0, a.shape[0])])

    def __len__(self):
        return sum(p[3] for p in self._parts)

    def __add__(self, other):
        if not isinstance(other, AudioFilter):
            return NotImplemented
        return AudioFilter(self._parts + other._parts)

    def sections(self, A):
        """float64 [S][6] for audio rows of A samples.  ValueError for a corner at or above A / 2, and for ``sos`` parts made
        for another rate."""
        A = int(A)
        got = self._sections.get(A)
        if got is None:
            rows = []
            for kind, arg, order, _ in self._parts:
                if kind == "sos":
                    if arg[1] != A:
                        raise ValueError("sos sections were designed for rows of %d samples, not %d" % (arg[1], A))
                    rows.append(arg[0])
                elif kind == "deemphasis":
                    K = _corner(1.0 / (2.0 * np.pi * arg[0]), A, kind) / (2.0 * A)      # tan(pi f_c / A)
                    rows.append(np.array([[K / (1.0 + K), K / (1.0 + K), 0.0, 1.0, (K - 1.0) / (K + 1.0), 0.0]]))
                else:
                    rows.append(_butter(kind, arg, order, A))
            got = _check_sos(np.ascontiguousarray(np.concatenate(rows), dtype=np.float64))
            got.setflags(write=False)
            self._sections[A] = got
        return got

    def _create(self, C, ch, A):
        """A new librcfm handle (zero state) for C channels of ch legs at rows of A samples."""
        sos = self.sections(A)
        out = ctypes.c_void_p()
        lib = hip.lib()
        hip.check(lib.rcfm_audio_filter_create(int(C), int(ch), int(sos.shape[0]),
                                               sos.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(out)))
        return hip.Handle(out, lib.rcfm_audio_filter_destroy)

    def run(self, audio, first=0, select=None):
        """Filters a device tensor ``audio`` [count, A] or [count, A, 2] in place, on the current stream, unsynchronised,
        with the states of channels ``first .. first + count - 1`` of this object's handle for (first + count, legs, A),
        made on first use.  ``select``: a device uint8 tensor [count], rows with 0 are left alone.  Returns ``audio``."""
        t = hip.torch()
        if audio.dim() not in (2, 3) or audio.dtype != t.float32 or not audio.is_contiguous() or \
                (audio.dim() == 3 and int(audio.shape[2]) not in (1, 2)):
            raise ValueError("audio is a contiguous float32 tensor [count, A] or [count, A, 2]")
        count, A = int(audio.shape[0]), int(audio.shape[1])
        ch = int(audio.shape[2]) if audio.dim() == 3 else 1
        if select is not None and (select.dtype != t.uint8 or select.numel() != count or not select.is_contiguous()):
            raise ValueError("select is a contiguous uint8 tensor [count]")
        key = (int(first) + count, ch, A)
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = self._create(*key)
        hip.check(hip.lib().rcfm_audio_filter_run(h.value, int(first), count, A, hip.ptr(audio), hip.ptr(audio),
                                                  hip.ptr(select) if select is not None else None, hip.stream()))
        return audio

    def reset(self):
        """Every state of run()'s handles back to zero, on the current stream."""
        for h in self._handles.values():
            hip.check(hip.lib().rcfm_audio_filter_reset(h.value, hip.stream()))


VOICE_NFM = AudioFilter.highpass(300.0) + AudioFilter.lowpass(3000.0) + AudioFilter.deemphasis(750e-6)
VOICE_AM = AudioFilter.bandpass(300.0, 3400.0)
