"""The frame gate's definition (include/rcfm.h, "frame gate") in plain numpy: frame power in float64, the gate's state machine
and look-ahead, the sample-exact apply -- each a second time frame by frame and sample by sample (`*_restated`), to pin the
vectorised forms -- and the keyed-station buffers the Tuner tests run, with the margin their exact comparison rests on."""

import numpy as np

MARGIN_DB = 3.0          # the project's squelch margin: a model level this far from a threshold cannot be flipped by rounding


def frame_power(x, L):
    """float64 [rows, n // L]: the mean of |x|^2 over each frame of L samples of x [rows, n] (float32 or complex64), squares
    and sums in float64 on the values as they are.  The tail n mod L is not read."""
    x = np.asarray(x)
    rows, n = x.shape
    F = n // L
    v = x[:, :F * L].reshape(rows, F, L)
    if np.iscomplexobj(v):
        sq = v.real.astype(np.float64) ** 2 + v.imag.astype(np.float64) ** 2
    else:
        sq = v.astype(np.float64) ** 2
    return sq.sum(axis=2) / L


def ramp(R):
    """float32 [R]: 0.5 - 0.5 cos(pi (i + 1) / (R + 1)) in float64, rounded once."""
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(R, dtype=np.float64) + 1.0) / (R + 1.0))).astype(np.float32)


def dilate(g, lead):
    """g'[f] = g[f] | ... | g[min(f + lead, F - 1)] along the last axis."""
    g = np.asarray(g, dtype=bool)
    F = g.shape[-1]
    out = g.copy()
    for k in range(1, min(int(lead), F - 1) + 1):
        out[..., :F - k] |= g[..., k:]
    return out


def _thresholds(open_thr, close_thr, count):
    return (np.broadcast_to(np.asarray(open_thr, dtype=np.float32), (count,)),
            np.broadcast_to(np.asarray(close_thr, dtype=np.float32), (count,)))


def gate_run(state, power, open_thr, close_thr, hang, lead):
    """(frame_mask uint8 [count, F + 1], open_any uint8 [count], state int32 [count, 2]) from state int32 [count, 2] and
    power float32 [count, F]; thresholds float32, a scalar or one per row.  All channels at once, frame after frame."""
    state = np.asarray(state, dtype=np.int32)
    p = np.asarray(power, dtype=np.float32)
    count, F = p.shape
    to, tc = _thresholds(open_thr, close_thr, count)
    is_open, left = state[:, 0] != 0, state[:, 1].copy()
    g = np.zeros((count, F), bool)
    with np.errstate(invalid="ignore"):
        for f in range(F):
            a = p[:, f] >= to
            b = ~a & is_open & (p[:, f] >= tc)
            c = ~a & ~b & is_open
            dec, close = c & (left > 0), c & (left <= 0)
            left = np.where(a | b, np.int32(hang), np.where(dec, left - 1, left)).astype(np.int32)
            is_open = (is_open | a) & ~close
            g[:, f] = is_open
    mask = np.concatenate([state[:, :1] != 0, dilate(g, lead)], axis=1).astype(np.uint8)
    return mask, mask.any(axis=1).astype(np.uint8), np.stack([is_open.astype(np.int32), left], axis=1)


def gate_run_restated(state, power, open_thr, close_thr, hang, lead):
    """gate_run as include/rcfm.h words it: one channel after the other, frame by frame, the look-ahead as an OR over a
    window."""
    p = np.asarray(power, dtype=np.float32)
    count, F = p.shape
    to, tc = _thresholds(open_thr, close_thr, count)
    mask = np.zeros((count, F + 1), np.uint8)
    any_ = np.zeros(count, np.uint8)
    new = np.zeros((count, 2), np.int32)
    for c in range(count):
        is_open, left = int(state[c][0] != 0), int(state[c][1])
        mask[c, 0] = is_open
        g = []
        for f in range(F):
            v = p[c, f]
            if v >= to[c]:
                is_open, left = 1, int(hang)
            elif is_open and v >= tc[c]:
                left = int(hang)
            elif is_open:
                if left > 0:
                    left -= 1
                else:
                    is_open = 0
            g.append(is_open)
        for f in range(F):
            mask[c, f + 1] = int(any(g[f:min(f + int(lead), F - 1) + 1]))
        any_[c] = int(mask[c].any())
        new[c] = (is_open, left)
    return mask, any_, new


def gate_apply(audio, mask, r):
    """The audio [count, A] or [count, A, ch] float32 behind rcfm_gate_apply with frame_mask `mask` [count, F + 1] and the
    ramp r float32 [R]: a new array; every product is one float32 multiply."""
    x = np.array(audio, dtype=np.float32)
    m = np.asarray(mask) != 0
    count, A = x.shape[:2]
    F, R = m.shape[1] - 1, int(len(r))
    La = A // F
    assert La * F == A and R <= La
    g, gp = np.repeat(m[:, 1:], La, axis=1), np.repeat(m[:, :-1], La, axis=1)          # [count, A]
    pos = np.tile(np.arange(La), F)
    inside = np.broadcast_to(pos < R, (count, A))
    up = np.zeros(A, np.float32)
    down = np.zeros(A, np.float32)
    up[pos < R] = r[pos[pos < R]]
    down[pos < R] = r[R - 1 - pos[pos < R]]
    shape = (count, A) + (1,) * (x.ndim - 2)
    gain = np.ones((count, A), np.float32)
    rise, fall = g & ~gp & inside, ~g & gp & inside
    gain[rise] = np.broadcast_to(up, (count, A))[rise]
    gain[fall] = np.broadcast_to(down, (count, A))[fall]
    scaled = rise | fall
    zero = ~g & ~scaled
    with np.errstate(invalid="ignore"):
        y = np.where(scaled.reshape(shape), x * gain.reshape(shape), x)
    return np.where(zero.reshape(shape), np.float32(0.0), y).astype(np.float32)


def gate_apply_restated(audio, mask, r):
    """gate_apply sample by sample, the table of include/rcfm.h."""
    y = np.array(audio, dtype=np.float32)
    count, A = y.shape[:2]
    F, R = mask.shape[1] - 1, int(len(r))
    La = A // F
    for c in range(count):
        for f in range(F):
            g, gp = int(mask[c, f + 1] != 0), int(mask[c, f] != 0)
            for i in range(La):
                k = f * La + i
                if g and gp:
                    continue
                if not g and not gp:
                    y[c, k] = np.float32(0.0)
                elif g:
                    if i < R:
                        y[c, k] = y[c, k] * r[i]
                elif i < R:
                    y[c, k] = y[c, k] * r[R - 1 - i]
                else:
                    y[c, k] = np.float32(0.0)
    return y


def margin_db(power, open_thr, close_thr):
    """The smallest distance in dB of a model frame power [count, F] from the thresholds of its row (NaN thresholds, which
    keep a channel closed whatever the power, do not count)."""
    p = np.asarray(power, dtype=np.float64)
    worst = np.inf
    for thr in (open_thr, close_thr):
        t = np.broadcast_to(np.asarray(thr, dtype=np.float64), (p.shape[0],))[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.abs(10.0 * np.log10(p / t))
        worst = min(worst, float(np.nanmin(d)))
    return worst


# ---- the keyed stations of the Tuner tests -------------------------------------------------------------------------------

FRAMES, HANG, LEAD, RAMP = 10, 0.3, 1, 0.02     # the gate of the Tuner tests: frames of 100 ms, 3 frames of hang, 1 of look-ahead
NOISE = 1e-4


class Scene:
    """Stations keyed on and off at frame boundaries: chans [(centre Hz, bandwidth)], keyed[c] the [first, last] runs of
    frames -- counted through all the buffers -- station c transmits in, amplitude[c] its carrier's, kind its modulation:
    "FM" (constant envelope), "AM", or "CW" (a bare carrier)."""

    def __init__(self, n, chans, keyed, amplitude, kind, buffers):
        self.n, self.chans, self.keyed, self.amplitude, self.kind, self.nbuf = n, chans, keyed, amplitude, kind, buffers
        self.C = len(chans)

    def add_to(self, tuner, demod=lambda B: None, order=None):
        """The channels on a Tuner (ours or the oracle's), `order`: station indices in the order they become channels."""
        for c in (range(self.C) if order is None else order):
            f, B = self.chans[c]
            tuner.add_channel(f, B, demod(B))
            tuner.request_bandwidth(float(self.n))
        return tuner

    def thresholds(self):
        """(open, close) float32 [C]: 10 dB and 13 dB below each station's carrier power."""
        a2 = np.array(self.amplitude, dtype=np.float64) ** 2
        return (0.1 * a2).astype(np.float32), (0.05 * a2).astype(np.float32)

    def keying(self):
        """bool [C, buffers FRAMES]: station c is keyed in frame f."""
        k = np.zeros((self.C, FRAMES * self.nbuf), bool)
        for c, runs in enumerate(self.keyed):
            for lo, hi in runs:
                k[c, lo:hi + 1] = True
        return k

    def buffers(self, f_in):
        """The complex64 [n] buffers: every station at its channel's centre, keyed, in a little noise."""
        rng = np.random.default_rng(20)
        n = self.n
        k = np.repeat(self.keying(), n // FRAMES, axis=1).astype(np.float64)
        t = np.arange(n, dtype=np.float64) / n
        out = []
        for b in range(self.nbuf):
            x = NOISE * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
            for c, (f, B) in enumerate(self.chans):
                tone = 2.0 * np.pi * (100.0 + 20.0 * c) * t
                carrier = 2.0 * np.pi * round(f - f_in) * t
                if self.kind == "FM":               # Carson bandwidth 2 (0.5 + 1) 240 Hz: well inside a channel of 2 kHz
                    s = np.exp(1j * (carrier + 0.5 * np.sin(tone)))
                elif self.kind == "AM":             # mean power 1
                    s = (1.0 + 0.5 * np.cos(tone)) / np.sqrt(1.125) * np.exp(1j * carrier)
                else:
                    s = np.exp(1j * carrier)
                x += self.amplitude[c] * k[c, b * n:(b + 1) * n] * s
            out.append(x.astype(np.complex64))
        return out

    def powers(self, ref, xs):
        """([float32 [C, FRAMES]] per buffer, the worst distance in dB of any of them from its thresholds): the model's frame
        powers of the oracle tuner's channel samples, in float64."""
        to, tc = self.thresholds()
        out, worst = [], np.inf
        for x in xs:
            ref.load(x.astype(np.complex128))
            p = np.concatenate([frame_power(np.asarray(ref.run(c))[None], B // FRAMES) for c, (_, B) in enumerate(self.chans)])
            worst = min(worst, margin_db(p, to, tc))
            out.append(p.astype(np.float32))
        return out, worst

    def masks(self, powers, stations=None, state=None):
        """([frame_mask [count, FRAMES + 1]], [open_any [count]]) per buffer of `powers`: the gate of the Tuner tests over the
        stations `stations` (all), from `state` (closed)."""
        idx = np.arange(self.C) if stations is None else np.asarray(stations)
        to, tc = self.thresholds()
        state = np.zeros((len(idx), 2), np.int32) if state is None else state
        masks, anys = [], []
        for p in powers:
            m, a, state = gate_run(state, p[idx], to[idx], tc[idx], int(round(HANG * FRAMES)), LEAD)
            masks.append(m)
            anys.append(a)
        return masks, anys


def _fall(top_db, C):
    return [0.5 * 10.0 ** (-top_db * c / max(C - 1, 1) / 20.0) for c in range(C)]


NARROW_KEYED = [
    [(0, 29)],                  # always there
    [],                         # never: noise only
    [(3, 6)],                   # inside the first buffer: opens one frame early, hangs three frames
    [(8, 12)],                  # across the first buffer edge
    [(0, 9)],                   # ends exactly at the buffer edge: the hang and the fade-out lie in the next buffer
    [(10, 14)],                 # starts with a buffer's first frame: nothing to look ahead from
    [(2, 3), (6, 7), (22, 22)], # a pause shorter than the hang time is bridged; a single frame late on
    [(25, 29)],                 # open when the last buffer ends
]


def narrow(kind):
    """N = 40 000, 8 channels of 2000 samples (audio 800), three buffers, levels over 20 dB."""
    return Scene(40000, [(100.0e6 + 2000.0 * (c - 4) + 1000.0, 2000) for c in range(8)], NARROW_KEYED, _fall(20.0, 8), kind, 3)


def mixed():
    """N = 40 000, four channels of 2000 samples below the centre and two of 4000 above it, two buffers."""
    chans = [(100.0e6 - 7000.0 + 2000.0 * c, 2000) for c in range(4)] + [(100.0e6 + 2000.0, 4000), (100.0e6 + 6000.0, 4000)]
    return Scene(40000, chans, [[(0, 19)], [(3, 6)], [], [(8, 12)], [(2, 4)], [(9, 13)]], _fall(15.0, 6), "FM", 2)


def stereo():
    """N = 600 000, three broadcast channels of 60 000 samples (bare carriers), two buffers."""
    chans = [(100.00e6, 60000), (100.05e6, 60000), (99.90e6, 60000)]
    return Scene(600000, chans, [[(0, 19)], [(4, 6), (18, 19)], []], [0.5, 0.3, 0.2], "CW", 2)
