"""Audio buses: the open channels mixed to a few mono or stereo streams on the device (rcfm_mix_*, include/rcfm.h, "audio
buses"; no reference counterpart).  A ``Bus`` is a list of routes -- a channel index and a left and a right gain each -- a
``Mixer`` a list of buses; ``Tuner.set_mix`` runs one behind everything else ``run_all`` / ``run_each`` queue, on the final
open mask, and ``Tuner.run_all_packed(pcm, drain=..., buses=True)`` packs and drains the bus rows instead of the channel rows:

    tower = Bus.of([3, 4, 7], gain_db=0.0, pan=[-0.6, 0.0, 0.6], name="tower")
    rest = Bus.of([c for c in range(760) if c not in (3, 4, 7)], gain_db=-6.0, name="rest")
    tuner.set_mix(Mixer([tower, rest]))
    tuner.load(x); tuner.run_all(); left_right = tuner.mix()       # [2, A, 2]
"""

import ctypes
import math

import numpy as np

from radiocore._internal import hip

__all__ = ["Bus", "Mixer"]


def pan_gains(g, pan):
    """Constant-power pan of a mono source, float64: ``(g cos((p + 1) pi / 4), g sin((p + 1) pi / 4))``, p in [-1, 1]."""
    theta = (np.asarray(pan, dtype=np.float64) + 1.0) * (math.pi / 4.0)
    return g * np.cos(theta), g * np.sin(theta)


def balance_gains(g, balance):
    """Balance of a stereo source, float64: ``(g min(1, 1 - p), g min(1, 1 + p))``, p in [-1, 1]."""
    p = np.asarray(balance, dtype=np.float64)
    return g * np.minimum(1.0, 1.0 - p), g * np.minimum(1.0, 1.0 + p)


class Bus:
    """``Bus(routes, name=None)``: one mixed output.  ``routes``: a list of ``(channel_index, gl, gr)`` -- the channel's
    index in ``Tuner.channels()`` and the float32 gains it enters the left and the right side with (a mono bus adds
    ``gl x`` of a mono channel and ``gl x_left + gr x_right`` of a stereo one).  The order of the routes is the order of
    the sum.  ValueError for a route of another form, a negative or repeated channel index, a gain that is not finite as
    float32, or more than 65 535 routes."""

    def __init__(self, routes, name=None):
        routes = list(routes)
        if len(routes) > hip.RCFM_MIX_MAX_BUS_ROUTES:
            raise ValueError("a bus takes at most %d routes, not %d" % (hip.RCFM_MIX_MAX_BUS_ROUTES, len(routes)))
        chans = np.zeros(len(routes), np.int32)
        gains = np.zeros((len(routes), 2), np.float32)
        for j, r in enumerate(routes):
            try:
                c, gl, gr = r
                ok = int(c) == c
                with np.errstate(over="ignore"):
                    gains[j] = (float(gl), float(gr))
            except (TypeError, ValueError):
                raise ValueError("a route is (channel_index, gl, gr), not %r" % (r,))
            if not ok or int(c) < 0 or int(c) > 2 ** 31 - 1:
                raise ValueError("a route's channel is an index from 0 up, not %r" % (c,))
            chans[j] = int(c)
        if not np.all(np.isfinite(gains)):
            raise ValueError("a route's gains are finite float32 numbers")
        if np.unique(chans).size != chans.size:
            raise ValueError("a channel appears at most once per bus")
        self.channels = chans
        self.gains = gains
        self.name = name

    @classmethod
    def of(cls, channels, gain_db=0.0, pan=0.0, balance=None, name=None):
        """A bus of ``channels`` (indices), each at ``gain_db`` dB -- one figure for all or one per channel -- and placed
        from left (-1) to right (+1): ``pan`` is the constant-power law for mono sources, ``gl = g cos((p + 1) pi / 4)``,
        ``gr = g sin((p + 1) pi / 4)``; ``balance=`` instead is the stereo (WBFM) form, ``gl = g min(1, 1 - p)``,
        ``gr = g min(1, 1 + p)``.  The gains are computed in float64 and rounded once to float32."""
        chans = [c for c in np.atleast_1d(np.asarray(channels)).tolist()] if np.size(channels) else []
        n = len(chans)

        def per_channel(a, what):
            a = np.asarray(a, dtype=np.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
                raise ValueError("%s: one for all or one per channel (%d)" % (what, n))
            if not np.all(np.isfinite(a)):
                raise ValueError("%s: finite numbers" % what)
            return np.broadcast_to(a, (n,))
        g = 10.0 ** (per_channel(gain_db, "gain_db") / 20.0)
        if balance is not None:
            if np.any(np.asarray(pan) != 0.0):
                raise ValueError("Bus.of takes pan or balance, not both")
            p, law = per_channel(balance, "balance"), balance_gains
        else:
            p, law = per_channel(pan, "pan"), pan_gains
        if np.any(np.abs(p) > 1.0):
            raise ValueError("pan and balance lie in [-1, 1]")
        gl, gr = law(g, p)
        with np.errstate(over="ignore"):
            gl, gr = gl.astype(np.float32), gr.astype(np.float32)
        return cls(list(zip(chans, gl.tolist(), gr.tolist())), name=name)

    def __len__(self):
        return int(self.channels.shape[0])

    def __repr__(self):
        return "Bus(%s%d routes)" % ("%r, " % (self.name,) if self.name is not None else "", len(self))


class Mixer:
    """``Mixer(buses, stereo=True)``: 1 .. 1024 buses with at most 2**20 routes in all; ``stereo=False`` makes the buses
    mono.  A settings object: it needs no device, and one mixer may serve several tuners."""

    def __init__(self, buses, stereo=True):
        buses = list(buses)
        if not 1 <= len(buses) <= hip.RCFM_MIX_MAX_BUSES:
            raise ValueError("a mixer takes 1 .. %d buses, not %d" % (hip.RCFM_MIX_MAX_BUSES, len(buses)))
        for b in buses:
            if not isinstance(b, Bus):
                raise ValueError("a mixer takes radiocore.Bus objects, not %r" % (b,))
        if sum(len(b) for b in buses) > hip.RCFM_MIX_MAX_ROUTES:
            raise ValueError("a mixer takes at most %d routes in all" % hip.RCFM_MIX_MAX_ROUTES)
        self.buses = tuple(buses)
        self.ch_out = 2 if stereo else 1

    @property
    def M(self):
        return len(self.buses)

    def highest_channel(self):
        """The greatest channel index any route names, -1 without a route."""
        return max([int(b.channels.max()) for b in self.buses if len(b)], default=-1)

    def _split(self, ranges, C):
        """The buses dealt to the launch groups ``ranges`` [(first, count)] of a tuner with C channels:
        ``(owner, tables)`` -- owner[m] the group bus m belongs to (0 for an empty bus), tables[k] = (bus_start int32
        [M + 1], channel int32 [R_k], gain float32 [R_k, 2]) of group k, in which the buses of other groups are empty.
        ValueError for a route to a channel the tuner does not have and for a bus whose channels lie in two groups."""
        owner = []
        for m, b in enumerate(self.buses):
            what = "bus %d" % m if b.name is None else "bus %r" % (b.name,)
            if len(b) and int(b.channels.max()) >= C:
                raise ValueError("%s routes channel %d, the tuner has %d channels" % (what, int(b.channels.max()), C))
            inside = [k for k, (f, n) in enumerate(ranges) if np.any((b.channels >= f) & (b.channels < f + n))]
            covered = sum(int(np.count_nonzero((b.channels >= f) & (b.channels < f + n))) for f, n in ranges)
            if covered != len(b):
                raise ValueError("%s routes a channel outside the channels this run covers" % what)
            if len(inside) > 1:
                raise ValueError("%s spans channels of different launch groups (class, geometry or bandwidth differ): "
                                 "a bus mixes channels of one group" % what)
            owner.append(inside[0] if inside else 0)
        tables = []
        for k in range(len(ranges)):
            mine = [b if owner[m] == k else None for m, b in enumerate(self.buses)]
            start = np.zeros(self.M + 1, np.int32)
            start[1:] = np.cumsum([len(b) if b is not None else 0 for b in mine])
            chan = np.concatenate([b.channels for b in mine if b is not None] + [np.zeros(0, np.int32)]).astype(np.int32)
            gain = np.concatenate([b.gains for b in mine if b is not None] + [np.zeros((0, 2), np.float32)]).astype(np.float32)
            tables.append((start, chan, gain))
        return owner, tables

    def _create(self, start, chan, gain):
        """A new librcfm handle for one group's tables."""
        out = ctypes.c_void_p()
        lib = hip.lib()
        ip = ctypes.POINTER(ctypes.c_int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        # (a group without a route still hands over addressable tables: one unused entry each)
        chan = np.ascontiguousarray(chan if chan.size else np.zeros(1), dtype=np.int32)
        gain = np.ascontiguousarray(gain if gain.size else np.zeros((1, 2)), dtype=np.float32)
        hip.check(lib.rcfm_mix_create(self.M, start.ctypes.data_as(ip), chan.ctypes.data_as(ip),
                                      gain.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), self.ch_out, ctypes.byref(out)))
        return hip.Handle(out, lib.rcfm_mix_destroy)
