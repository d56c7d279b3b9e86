"""The bus dynamics of include/rcfm.h ("bus dynamics", rcfm_busdyn_*) in numpy: the model the device must equal bit for bit, a
sample-by-sample scalar restatement of the same definition, three deliberately wrong models (what a kernel that took a
shortcut would compute), and the seeded inputs tests/test_hip_busdyn.py runs the kernels on.

numpy's float32 multiply, add, subtract and divide are single IEEE operations, round to nearest, and separate ufunc calls are
never fused: the ``(x) (+) (-) (/)`` of the definition."""

import numpy as np

F32 = np.float32
TINY = np.finfo(np.float32).tiny


def _max(v, p):
    """v > p ? v : p -- a NaN v never wins."""
    return np.where(v > p, v, p)


def _min(a, b):
    """b < a ? b : a"""
    return np.where(b < a, b, a)


def _fma(a, b, c):
    # a b + c with one rounding to float32, near enough: the product of two float32 is exact in float64
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


class Params:
    """What a handle has: M buses of ch legs, block length L, ceiling c, release coefficient k, and the duck tables (or None)."""

    def __init__(self, M, ch, L, c, k, key=None, depth=None, thr=None, hold=None):
        self.M, self.ch, self.L = int(M), int(ch), int(L)
        self.c, self.k = F32(c), F32(k)
        self.key = None if key is None else np.asarray(key, np.int32)
        self.depth = None if key is None else np.asarray(depth, F32)
        self.thr = None if key is None else np.asarray(thr, F32)
        self.hold = None if key is None else np.asarray(hold, np.int32)

    def tables(self):
        return self.key, self.depth, self.thr, self.hold


class State:
    """tail [M, L, ch] float32, h [M] float32, hang [M] int32; the reset values by default."""

    def __init__(self, p, tail=None, h=None, hang=None):
        self.tail = np.zeros((p.M, p.L, p.ch), F32) if tail is None else tail
        self.h = np.ones(p.M, F32) if h is None else h
        self.hang = np.zeros(p.M, np.int32) if hang is None else hang


def block_peaks(ext, L, A):
    """P [M, B + 1] float32: P[:, 0] = Pk[-1], the peak of the tail, P[:, j + 1] = Pk[j]."""
    a = np.fmax.reduce(np.abs(ext), axis=-1, initial=F32(0))                 # fmax passes a NaN over, like v > p ? v : p
    tail = np.fmax.reduce(a[:, :L], axis=1, initial=F32(0))
    row = np.fmax.reduceat(a[:, L:], np.arange(0, A, L), axis=1)
    return np.fmax(np.concatenate([tail[:, None], row], axis=1), F32(0)).astype(F32)    # a block of NaNs only peaks at +0


def run(p, st, x, open_in=None, watch=None, variant=None):
    """One call: (out [M, A, ch] float32, bus_open_out uint8 [M], the new State) of x [M, A, ch] and the State before it.
    Vectorised over buses and samples; the knots are walked in order.  ``watch(array)`` is called with every intermediate
    product, sum and difference (the denormal check).  ``variant``: None, or one of the WRONG models below."""
    x = np.asarray(x, F32)
    M, A, ch = x.shape
    L, c, k, one = p.L, p.c, p.k, F32(1)
    assert (M, ch) == (p.M, p.ch) and A >= 1
    ext = np.concatenate([st.tail, x], axis=1)
    P = block_peaks(ext, L, A)
    B = P.shape[1] - 1
    H = np.zeros((M, B + 1), F32)
    h, hang = st.h.astype(F32), st.hang.astype(np.int32)
    H[:, 0] = h
    see = watch if watch is not None else (lambda a: None)
    for b in range(1, B + 1):
        Q = P[:, b] if variant == "no look-ahead" else _max(P[:, b], P[:, b - 1])
        T = np.divide(c, Q, out=np.ones(M, F32), where=Q > c)
        if p.key is not None:
            keyed = p.key >= 0
            kk = np.where(keyed, p.key, 0)
            Qk = _max(P[kk, b], P[kk, b - 1])
            hit = keyed & (Qk > p.thr)
            hanging = keyed & ~hit & (hang > 0)
            hang = np.where(hit, p.hold, np.where(hanging, hang - 1, hang)).astype(np.int32)
            T = np.where(hit | hanging, _min(T, p.depth), T)
        if variant == "fma":
            r = _fma(one - h, k, h)
        elif variant == "float64 release":
            r = (h.astype(np.float64) + (1.0 - h.astype(np.float64)) * np.float64(k)).astype(F32)
        else:
            r = h + (one - h) * k
            see(one - h), see((one - h) * k), see(r)
        h = _min(T, r).astype(F32)
        H[:, b] = h
    n = np.arange(A)
    j = n // L
    i = n - j * L
    w = (i + 1).astype(F32) / np.minimum(L, A - j * L).astype(F32)
    h0, h1 = H[:, j], H[:, j + 1]
    if variant == "fma":
        g = _fma(h1 - h0, w, h0)
    else:
        g = h0 + (h1 - h0) * w
        see(h1 - h0), see((h1 - h0) * w), see(g)
    y = ext[:, :A] * g[:, :, None]
    see(y)
    out = np.where(y > c, c, np.where(y < -c, -c, y)).astype(F32)
    open_out = np.ones(M, np.uint8) if open_in is None else ((np.asarray(open_in) != 0) | (P[:, 0] > 0)).astype(np.uint8)
    return out, open_out, State(p, ext[:, A:A + L].copy(), h, hang)


def run_restated(p, st, x, open_in=None):
    """The definition once more, one bus, one knot and one sample at a time, in scalar float32.  For small inputs."""
    x = np.asarray(x, F32)
    M, A, ch = x.shape
    L, c, k = p.L, F32(p.c), F32(p.k)
    B = -(-A // L)
    edge = [min(j * L, A) for j in range(B + 1)]

    def peak(ext, lo, hi):
        q = F32(0)
        for n in range(lo, hi):
            for leg in range(ch):
                v = F32(abs(ext[n + L, leg]))
                q = v if v > q else q
        return q
    exts = [np.concatenate([st.tail[m], x[m]], axis=0) for m in range(M)]
    Pk = [[peak(exts[m], -L, 0)] + [peak(exts[m], edge[j], edge[j + 1]) for j in range(B)] for m in range(M)]     # Pk[m][j + 1]
    out = np.zeros((M, A, ch), F32)
    new = State(p)
    open_out = np.zeros(M, np.uint8)
    for m in range(M):
        h, hang = [F32(st.h[m])], int(st.hang[m])
        for b in range(1, B + 1):
            Q = Pk[m][b] if Pk[m][b] > Pk[m][b - 1] else Pk[m][b - 1]
            T = F32(c / Q) if Q > c else F32(1)
            if p.key is not None and p.key[m] >= 0:
                key = int(p.key[m])
                Qk = Pk[key][b] if Pk[key][b] > Pk[key][b - 1] else Pk[key][b - 1]
                if Qk > p.thr[m]:
                    hang, on = int(p.hold[m]), True
                elif hang > 0:
                    hang, on = hang - 1, True
                else:
                    on = False
                if on and p.depth[m] < T:
                    T = F32(p.depth[m])
            r = F32(h[-1] + F32(F32(F32(1) - h[-1]) * k))
            h.append(T if T < r else r)
        for n in range(A):
            j = n // L
            w = F32(F32(n - j * L + 1) / F32(edge[j + 1] - edge[j]))
            g = F32(h[j] + F32(F32(h[j + 1] - h[j]) * w))
            for leg in range(ch):
                y = F32(exts[m][n, leg] * g)
                out[m, n, leg] = c if y > c else (-c if y < -c else y)
        new.tail[m] = exts[m][A:A + L]
        new.h[m], new.hang[m] = h[B], hang
        open_out[m] = 1 if open_in is None else int(open_in[m] != 0 or Pk[m][0] > 0)
    return out, open_out, new


# Three wrong models: the interpolation and the release step as an fma; the release step in float64; no look-ahead.
WRONG = ("fma", "float64 release", "no look-ahead")


def pcm_s16(x, gain=32767.0):
    """RCFM_PCM_S16 of include/rcfm.h: one float32 multiply, NaN -> 0, round to nearest even, clamp to +-32767."""
    y = np.asarray(x, F32) * F32(gain)
    return np.rint(np.clip(np.nan_to_num(y, nan=0.0), -32767.0, 32767.0)).astype(np.int16)


# ---- the float64 discretisation of radiocore.Limiter and radiocore.Duck -----------------------------------------------

def limiter_params(rate, ceiling_db=-1.0, lookahead=0.008, release=0.25):
    """(L, c, k) at the audio rate ``rate``: float64, each rounded once."""
    L = int(min(max(round(lookahead * rate), 8), 2048))
    return L, F32(10.0 ** (ceiling_db / 20.0)), F32(1.0 - np.exp(-L / (release * rate)))


def duck_params(rate, L, depth_db=-12.0, threshold_db=-40.0, hold=0.5):
    """(d, thr, hold in blocks) at the audio rate ``rate`` and block length L."""
    return F32(10.0 ** (depth_db / 20.0)), F32(10.0 ** (threshold_db / 20.0)), int(min(max(round(hold * rate / L), 0), 1 << 15))


# ---- inputs -----------------------------------------------------------------------------------------------------------

KINDS = ("burst", "steady", "below", "zero")


def make_input(rng, kind, A, ch, m=0, M=1):
    """One row [A, ch] float32: 0.1 sigma noise with a burst 30 x over it for an eighth of the call, placed by the bus; 1
    sigma noise, over the ceiling throughout; noise that stays below 0.8; or +0."""
    if kind == "zero":
        return np.zeros((A, ch), F32)
    if kind == "steady":
        return rng.standard_normal((A, ch)).astype(F32)
    x = (0.1 * rng.standard_normal((A, ch))).astype(F32)
    if kind == "below":
        return np.clip(x, F32(-0.8), F32(0.8))
    n = max(A // 8, 1)
    at = (m * (A - n)) // max(M, 1)
    x[at:at + n] *= F32(30.0)
    return x


def burst_calls(seed, M, A, ch, calls=3):
    rng = np.random.default_rng(seed)
    return [np.stack([make_input(rng, "burst", A, ch, (m + q) % (M + 1), M + 1) for m in range(M)]) for q in range(calls)]


# the three named burst inputs on which every wrong model must differ from the model: (M, A, ch, L)
BURSTS = {"burst 3x1000x2 L64": (3, 1000, 2, 64), "burst 3x1024x1 L64": (3, 1024, 1, 64), "burst 1x4099x1 L100": (1, 4099, 1, 100)}


def burst_case(name):
    M, A, ch, L = BURSTS[name]
    c = limiter_params(8000.0)[1]
    k = F32(1.0 - np.exp(-L / (0.25 * 8000.0)))                   # the default release at 8 kHz, for this block length
    return Params(M, ch, L, c, k), burst_calls(sum(map(ord, name)), M, A, ch)


class Case:
    """One sequence of rcfm_busdyn_run calls: the handle's parameters, the inputs and open masks of three calls, and the
    model's outputs and states after each, made once."""

    def __init__(self, name, seed, M, A, ch, L, kinds, duck=None, masked=True, c=None, k=None):
        rng = np.random.default_rng(seed)
        self.name, self.A = name, A
        c = F32(10.0 ** (-1.0 / 20.0)) if c is None else c
        k = F32(1.0 - np.exp(-L / (0.25 * 8000.0))) if k is None else k
        self.p = Params(M, ch, L, c, k, *(duck if duck is not None else (None,) * 4))
        self.x, self.open = [], []
        for q in range(3):
            self.x.append(np.stack([make_input(rng, kinds[(m + q) % len(kinds)], A, ch, m, M) for m in range(M)]))
            self.open.append((rng.random(M) < 0.5).astype(np.uint8) * rng.integers(1, 256, size=M).astype(np.uint8) if masked else None)
        self._want = None

    def want(self, watch=None):
        """[(out, bus_open_out, State)] after each call."""
        if self._want is None or watch is not None:
            st, got = State(self.p), []
            for x, o in zip(self.x, self.open):
                out, open_out, st = run(self.p, st, x, o, watch=watch)
                got.append((out, open_out, st))
            self._want = got
        return self._want


def _duck(M, rng, hold):
    key = np.array([(m + 1) % M if m % 2 == 0 and M > 1 else -1 for m in range(M)], np.int32)
    return key, rng.uniform(0.1, 0.9, M).astype(F32), rng.uniform(0.0, 0.5, M).astype(F32), np.full(M, hold, np.int32)


def _cases():
    out, seed = [], 900
    mixed = ("burst", "steady", "below", "zero")
    for A in (1, 5, 63, 64, 65, 1000, 4099):
        for L in (8, 64, 100):
            for ch in (1, 2):
                seed += 1
                rng = np.random.default_rng(seed)
                duck = _duck(3, rng, 2) if (A + L + ch) % 2 else None
                out.append(Case("sweep A=%d L=%d ch=%d" % (A, L, ch), seed, 3, A, ch, L, mixed, duck=duck))
    for ch in (1, 2):
        out.append(Case("L=2048 ch=%d" % ch, 950 + ch, 3, 1000, ch, 2048, mixed))
    for M in (1, 3, 64):
        for ch in (1, 2):
            rng = np.random.default_rng(960 + M + ch)
            out.append(Case("M=%d ch=%d" % (M, ch), 960 + M + ch, M, 1000, ch, 64, mixed, duck=_duck(M, rng, 3) if M > 1 else None))
    for kind in KINDS:
        out.append(Case("all %s" % kind, 980 + len(kind), 3, 1000, 2, 64, (kind,)))
        out.append(Case("all %s, ducked" % kind, 985 + len(kind), 3, 1000, 2, 64, (kind,), duck=_duck(3, np.random.default_rng(7), 2)))
    rng = np.random.default_rng(990)
    hold0 = _duck(3, rng, 0)
    out.append(Case("hold = 0", 991, 3, 1000, 1, 64, ("burst", "below", "zero"), duck=hold0))
    chain = (np.array([-1, 0, 1, 2], np.int32), np.array([1.0, 0.5, 0.25, 0.7], F32), np.array([0.0, 0.3, 0.05, 0.0], F32),
             np.array([0, 1, 4, 2], np.int32))
    out.append(Case("key chain", 992, 4, 1000, 2, 64, ("burst", "below", "below", "steady"), duck=chain))
    out.append(Case("open NULL", 993, 3, 1000, 2, 64, mixed, masked=False))
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
