"""Bus dynamics: a look-ahead peak limiter and ducking behind the mixer (rcfm_busdyn_*, include/rcfm.h, "bus dynamics"; no
reference counterpart).  ``Limiter`` and ``Duck`` are settings in dB and seconds, discretised per audio rate;
``Tuner.set_bus_dynamics`` runs them on the buses of ``Tuner.set_mix``:

    tuner.set_mix(Mixer([tower, rest]))
    tuner.set_bus_dynamics(Limiter(ceiling_db=-1.0), ducks={"rest": Duck("tower", depth_db=-12.0)})
    tuner.load(x); tuner.run_all(); left_right = tuner.mix()       # [2, A, 2], limited, L samples late (tuner.bus_delay())
"""

import ctypes
import math

import numpy as np

from radiocore._internal import hip

__all__ = ["Limiter", "Duck"]


def _finite(value, what):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s is a number, not %r" % (what, value))
    if not math.isfinite(v):
        raise ValueError("%s is finite, not %r" % (what, value))
    return v


class Limiter:
    """``Limiter(ceiling_db=-1.0, lookahead=0.008, release=0.25)``: no output sample exceeds the ceiling (dB re full scale);
    the gain starts down ``lookahead`` seconds before a peak arrives -- which is also the delay of the bus -- and recovers
    with the time constant ``release`` seconds.  A settings object: it needs no device.  ValueError for a number that is
    not finite and for a look-ahead or release that is not above 0."""

    def __init__(self, ceiling_db=-1.0, lookahead=0.008, release=0.25):
        self.ceiling_db = _finite(ceiling_db, "ceiling_db")
        self.lookahead = _finite(lookahead, "lookahead")
        self.release = _finite(release, "release")
        if self.lookahead <= 0.0 or self.release <= 0.0:
            raise ValueError("lookahead and release are above 0 seconds")
        with np.errstate(over="ignore"):
            c = np.float32(10.0 ** (self.ceiling_db / 20.0))
        if not (np.isfinite(c) and c > 0):
            raise ValueError("the ceiling %g dB is no finite float32 above 0" % self.ceiling_db)

    def discretise(self, rate):
        """``(L, c, k)`` at the audio rate ``rate`` (Hz; buffers are one second long, so a row of A samples has the rate
        A), computed in float64 and rounded once: the block length ``L = clip(round(lookahead rate), 8, 2048)`` samples
        (halves to even), the ceiling ``c = 10 ** (ceiling_db / 20)`` and the release coefficient per block
        ``k = 1 - exp(-L / (release rate))`` as float32.  ValueError when k rounds to 0."""
        L = int(min(max(round(self.lookahead * float(rate)), hip.RCFM_BUSDYN_MIN_BLOCK), hip.RCFM_BUSDYN_MAX_BLOCK))
        k = np.float32(1.0 - math.exp(-L / (self.release * float(rate))))
        if not k > 0:
            raise ValueError("a release of %g s is too long for blocks of %d samples at %g Hz" % (self.release, L, rate))
        return L, np.float32(10.0 ** (self.ceiling_db / 20.0)), k

    def __repr__(self):
        return "Limiter(ceiling_db=%g, lookahead=%g, release=%g)" % (self.ceiling_db, self.lookahead, self.release)


class Duck:
    """``Duck(key, depth_db=-12.0, threshold_db=-40.0, hold=0.5)``: the bus this is set for is turned down to ``depth_db``
    (at most 0) while the bus ``key`` -- an index or a ``Bus`` name -- is above ``threshold_db`` (dB re full scale, peak) and
    for ``hold`` seconds after it has fallen silent; the limiter's look-ahead and release shape the way down and back."""

    def __init__(self, key, depth_db=-12.0, threshold_db=-40.0, hold=0.5):
        if isinstance(key, bool) or not isinstance(key, (int, np.integer, str)):
            raise ValueError("a duck's key is a bus index or a bus name, not %r" % (key,))
        self.key = key if isinstance(key, str) else int(key)
        self.depth_db = _finite(depth_db, "depth_db")
        self.threshold_db = _finite(threshold_db, "threshold_db")
        self.hold = _finite(hold, "hold")
        if self.depth_db > 0.0:
            raise ValueError("depth_db is at most 0 dB")
        if self.hold < 0.0:
            raise ValueError("hold is at least 0 seconds")
        with np.errstate(over="ignore"):
            d, thr = np.float32(10.0 ** (self.depth_db / 20.0)), np.float32(10.0 ** (self.threshold_db / 20.0))
        if not d > 0 or not np.isfinite(thr):
            raise ValueError("depth_db and threshold_db give finite float32 factors, the depth above 0")

    def discretise(self, rate, L):
        """``(d, thr, hold)`` for blocks of L samples at the audio rate ``rate``: the factors ``10 ** (dB / 20)`` as float32
        and the hold in blocks, ``clip(round(hold rate / L), 0, 2 ** 15)``."""
        blocks = int(min(max(round(self.hold * float(rate) / L), 0), hip.RCFM_BUSDYN_MAX_HOLD))
        return np.float32(10.0 ** (self.depth_db / 20.0)), np.float32(10.0 ** (self.threshold_db / 20.0)), blocks

    def __repr__(self):
        return "Duck(%r, depth_db=%g, threshold_db=%g, hold=%g)" % (self.key, self.depth_db, self.threshold_db, self.hold)


def resolve_ducks(ducks, buses):
    """int32 [M] key per bus (-1: none) and the Duck per bus, from ``{bus index or name: Duck}`` and the mixer's buses.
    ValueError for a bus or key that does not exist, a name that two buses carry, and a bus that is its own key."""
    M = len(buses)

    def index(ref, what):
        if isinstance(ref, str):
            hits = [m for m, b in enumerate(buses) if b.name == ref]
            if len(hits) != 1:
                raise ValueError("%s %r names %s" % (what, ref, "no bus" if not hits else "%d buses" % len(hits)))
            return hits[0]
        if isinstance(ref, bool) or not isinstance(ref, (int, np.integer)) or not 0 <= int(ref) < M:
            raise ValueError("%s %r is no bus of this mixer (0 .. %d, or a name)" % (what, ref, M - 1))
        return int(ref)
    key, per_bus = np.full(M, -1, np.int32), [None] * M
    for ref, duck in dict(ducks).items():
        if not isinstance(duck, Duck):
            raise ValueError("ducks maps a bus to a radiocore.Duck, not %r" % (duck,))
        m, km = index(ref, "the ducked bus"), index(duck.key, "the key")
        if per_bus[m] is not None:
            raise ValueError("bus %d is ducked twice" % m)
        if km == m:
            raise ValueError("bus %d cannot duck itself" % m)
        key[m], per_bus[m] = km, duck
    return key, per_bus


def create(M, ch, L, A_max, c, k, key=None, depth=None, thr=None, hold=None):
    """A new librcfm handle (rcfm_busdyn_create); the four duck tables or none."""
    out = ctypes.c_void_p()
    lib = hip.lib()
    ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    tables = (None, None, None, None)
    keep = ()
    if key is not None:
        keep = (np.ascontiguousarray(key, dtype=np.int32), np.ascontiguousarray(depth, dtype=np.float32),
                np.ascontiguousarray(thr, dtype=np.float32), np.ascontiguousarray(hold, dtype=np.int32))
        tables = (keep[0].ctypes.data_as(ip), keep[1].ctypes.data_as(fp), keep[2].ctypes.data_as(fp), keep[3].ctypes.data_as(ip))
    hip.check(lib.rcfm_busdyn_create(int(M), int(ch), int(L), int(A_max), float(c), float(k), *tables, ctypes.byref(out)))
    return hip.Handle(out, lib.rcfm_busdyn_destroy)
