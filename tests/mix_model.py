"""The audio buses of include/rcfm.h ("audio buses", rcfm_mix_*) in numpy: the model the device must equal bit for bit, a
route-by-route, sample-by-sample restatement of the same definition, the pan and balance laws of ``Bus.of`` in float64, three
deliberately wrong models (another order or another rounding: what a kernel that took a shortcut would compute), and the
seeded inputs tests/test_hip_mix.py runs the kernel on.

numpy's float32 multiply and add are single IEEE operations, round to nearest, and separate ufunc calls are never fused: the
``(x)`` and ``(+)`` of the definition."""

import numpy as np

SEGMENT = 16
F32 = np.float32


def _legs(x):
    """(x^L, x^R) of rows [.., A, ch_in]: the first and the last leg (the same when ch_in = 1)."""
    return x[..., 0], x[..., -1]


def _terms(x, gl, gr, ch_out):
    """[A, ch_out] float32: the terms of one route for the row x [A, ch_in]."""
    xl, xr = _legs(x)
    tl, tr = F32(gl) * xl, F32(gr) * xr
    if ch_out == 2:
        return np.stack([tl, tr], axis=-1)
    if x.shape[-1] == 1:
        return tl[:, None]
    return (tl + tr)[:, None]


def mix(audio, open_mask, first, bus_start, chan, gain, ch_out, segment=SEGMENT, watch=None):
    """(out [M, A, ch_out] float32, active int32 [M], bus_open uint8 [M]) of audio [count, A, ch_in] float32, the channels
    [first, first + count); open_mask: [count], nonzero = open, or None.  Vectorised over the samples.  ``watch(array)`` is
    called with every product and every partial sum (the denormal check)."""
    audio = np.asarray(audio, dtype=F32)
    M, A = len(bus_start) - 1, audio.shape[1]
    out = np.zeros((M, A, ch_out), F32)
    active = np.zeros(M, np.int32)
    for m in range(M):
        acc = np.zeros((A, ch_out), F32)
        lo, hi = int(bus_start[m]), int(bus_start[m + 1])
        for s0 in range(lo, hi, segment):
            s = np.zeros((A, ch_out), F32)
            for j in range(s0, min(s0 + segment, hi)):
                c = int(chan[j]) - first
                if open_mask is not None and not open_mask[c]:
                    continue                          # the row is not read
                active[m] += 1
                t = _terms(audio[c], gain[j][0], gain[j][1], ch_out)
                s = s + t
                if watch is not None:
                    xl, xr = _legs(audio[c])
                    for a in (F32(gain[j][0]) * xl, F32(gain[j][1]) * xr, t, s):
                        watch(a)
            acc = acc + s
            if watch is not None:
                watch(acc)
        out[m] = acc
    return out, active, (active > 0).astype(np.uint8)


def mix_restated(audio, open_mask, first, bus_start, chan, gain, ch_out):
    """The definition once more, one scalar at a time: per bus, output sample and leg, the segments in order, the open
    routes of each in order.  For small inputs."""
    audio = np.asarray(audio, dtype=F32)
    M, A, ch_in = len(bus_start) - 1, audio.shape[1], audio.shape[2]
    out = np.zeros((M, A, ch_out), F32)
    for m in range(M):
        routes = list(range(int(bus_start[m]), int(bus_start[m + 1])))
        segments = [routes[i:i + 16] for i in range(0, len(routes), 16)]
        for a in range(A):
            for leg in range(ch_out):
                total = F32(0.0)
                for seg in segments:
                    part = F32(0.0)
                    for j in seg:
                        c = int(chan[j]) - first
                        if open_mask is not None and open_mask[c] == 0:
                            continue
                        gl, gr = F32(gain[j][0]), F32(gain[j][1])
                        xl, xr = audio[c, a, 0], audio[c, a, ch_in - 1]
                        if ch_out == 2:
                            t = F32(gl * xl) if leg == 0 else F32(gr * xr)
                        elif ch_in == 1:
                            t = F32(gl * xl)
                        else:
                            t = F32(F32(gl * xl) + F32(gr * xr))
                        part = F32(part + t)
                    total = F32(total + part)
                out[m, a, leg] = total
    return out


# ---- three wrong models ----------------------------------------------------------------------------------------------

def mix_unsegmented(audio, open_mask, first, bus_start, chan, gain, ch_out):
    """WRONG on purpose: one left-to-right sum over all routes of a bus, no segments."""
    return mix(audio, open_mask, first, bus_start, chan, gain, ch_out, segment=1 << 30)[0]


def mix_segments_of_32(audio, open_mask, first, bus_start, chan, gain, ch_out):
    """WRONG on purpose: segments of 32 routes."""
    return mix(audio, open_mask, first, bus_start, chan, gain, ch_out, segment=32)[0]


def _fma(a, b, c):
    # a b + c with one rounding to float32, near enough: the product of two float32 is exact in float64
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def mix_fused(audio, open_mask, first, bus_start, chan, gain, ch_out):
    """WRONG on purpose: the product fused into the add that follows it (what contraction to an fma gives)."""
    audio = np.asarray(audio, dtype=F32)
    M, A = len(bus_start) - 1, audio.shape[1]
    out = np.zeros((M, A, ch_out), F32)
    for m in range(M):
        acc = np.zeros((A, ch_out), F32)
        lo, hi = int(bus_start[m]), int(bus_start[m + 1])
        for s0 in range(lo, hi, SEGMENT):
            s = np.zeros((A, ch_out), F32)
            for j in range(s0, min(s0 + SEGMENT, hi)):
                c = int(chan[j]) - first
                if open_mask is not None and not open_mask[c]:
                    continue
                xl, xr = _legs(audio[c])
                gl, gr = F32(gain[j][0]), F32(gain[j][1])
                if ch_out == 2:
                    s = np.stack([_fma(gl, xl, s[:, 0]), _fma(gr, xr, s[:, 1])], axis=-1)
                elif audio.shape[-1] == 1:
                    s = _fma(gl, xl, s[:, 0])[:, None]
                else:
                    s = (_fma(gr, xr, F32(gl) * xl) + s[:, 0])[:, None]
            acc = acc + s
        out[m] = acc
    return out


WRONG = {"unsegmented": mix_unsegmented, "fused": mix_fused, "segments of 32": mix_segments_of_32}


# ---- the gain laws of Bus.of, float64 ----------------------------------------------------------------------------------

def pan_gains(gain_db, pan):
    g = 10.0 ** (np.asarray(gain_db, np.float64) / 20.0)
    p = np.asarray(pan, np.float64)
    return g * np.cos((p + 1.0) * np.pi / 4.0), g * np.sin((p + 1.0) * np.pi / 4.0)


def balance_gains(gain_db, balance):
    g = 10.0 ** (np.asarray(gain_db, np.float64) / 20.0)
    p = np.asarray(balance, np.float64)
    return g * np.minimum(1.0, 1.0 - p), g * np.minimum(1.0, 1.0 + p)


def pcm_s16(x, gain=32767.0):
    """RCFM_PCM_S16 of include/rcfm.h: one float32 multiply, NaN -> 0, round to nearest even, clamp to +-32767."""
    y = np.asarray(x, F32) * F32(gain)
    r = np.rint(np.clip(np.nan_to_num(y, nan=0.0), -32767.0, 32767.0))
    return r.astype(np.int16)


# ---- the seeded inputs of the GPU test ---------------------------------------------------------------------------------

SWEEP_COUNTS = (0, 1, 15, 16, 17, 33, 100, 40, 64, 5)      # routes per bus; the last bus's channels are all closed
SWEEP_CHANNELS = 112
SWEEP_A = (1, 5, 64, 1000, 4099)


class Case:
    """One input of rcfm_mix_run: tables, audio [count, A, ch_in], mask (or None) and the model's outputs, made once."""

    def __init__(self, name, seed, counts, count, A, ch_in, ch_out, first=0, masked=True, closed_bus=None, nan_closed=False):
        rng = np.random.default_rng(seed)
        self.name, self.count, self.A, self.ch_in, self.ch_out, self.first = name, count, A, ch_in, ch_out, first
        self.M = len(counts)
        self.bus_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        reserved = np.arange(count - counts[closed_bus], count) if closed_bus is not None else np.zeros(0, np.int64)
        free = count - len(reserved)
        chans = []
        for m, n in enumerate(counts):
            chans.append(reserved if m == closed_bus else rng.choice(free, size=n, replace=False))
        self.chan = (np.concatenate(chans) + first).astype(np.int32) if chans else np.zeros(0, np.int32)
        R = int(self.bus_start[-1])
        db = rng.uniform(-12.0, 6.0, size=R)
        gl, gr = pan_gains(db, rng.uniform(-1.0, 1.0, size=R))
        self.gain = np.stack([gl, gr], axis=-1).astype(F32)
        self.audio = rng.standard_normal((count, A, ch_in)).astype(F32)
        self.open = None
        if masked:
            self.open = (rng.random(count) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=count).astype(np.uint8)
            self.open[reserved] = 0
        if nan_closed:
            self.audio[self.open == 0] = np.nan
        self._want = None

    def args(self):
        return self.audio, self.open, self.first, self.bus_start, self.chan, self.gain, self.ch_out

    def want(self):
        if self._want is None:
            self._want = mix(*self.args())
        return self._want


def _cases():
    out, seed = [], 400
    for A in SWEEP_A:
        for ch_in in (1, 2):
            for ch_out in (1, 2):
                seed += 1
                out.append(Case("sweep A=%d %d->%d" % (A, ch_in, ch_out), seed, SWEEP_COUNTS, SWEEP_CHANNELS, A, ch_in, ch_out,
                                closed_bus=len(SWEEP_COUNTS) - 1))
    out.append(Case("M=1", 31, (40,), 48, 1000, 1, 2))
    out.append(Case("M=3", 32, (40, 33, 50), 56, 1000, 1, 2))
    out.append(Case("M=64", 33, tuple(33 + m % 16 for m in range(64)), 64, 1000, 1, 2))
    out.append(Case("open NULL", 34, (40, 33, 50), 56, 64, 2, 2, masked=False))
    out.append(Case("first > 0", 35, (40, 33, 50), 56, 1000, 1, 2, first=7))
    out.append(Case("NaN in closed rows", 36, (40, 33, 36, 20), 64, 1000, 2, 2, closed_bus=3, nan_closed=True))
    # more than 8 segments: a workgroup's eight waves take a bus of more than 128 routes in several rounds
    out.append(Case("long buses 1->2", 37, (130, 300, 257, 129), 320, 64, 1, 2))
    out.append(Case("long buses 2->1", 38, (130, 300, 257, 129), 320, 69, 2, 1))
    return out


_CASES = None


def cases():
    """The inputs the GPU test compares exactly, made once per process."""
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)
