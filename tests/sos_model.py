"""Audio filter test model (no test functions): the biquad cascade of include/rcfm.h (rcfm_audio_filter_*) in numpy.

    per section, transposed direct form II:  y = b0 u + z0;  z0' = b1 u - a1 y + z1;  z1' = b2 u - a2 y
    section s + 1 reads section s; the state (z0, z1) per section is carried from call to call and starts at zero.

Three statements of it:
    truth       float64, sample after sample, a recurrence of its own (tests/test_sos_model.py holds it against
                scipy.signal.sosfilt with zi carried)
    yardstick   the same recurrence with every operation rounded to float32, vectorised over the rows.  Its distance from
                truth is what a float32 receiver costs; the GPU tests allow four times that, within 1e-6 .. 1e-4
    block       float64, in the form the kernel evaluates: segments of 8192, runs of 33 from zero state, the affine scan
                s_t = M^R s_(t-1) + v_(t-1) with M = [[-a1, 1], [-a2, 0]], the runs again from s_t, one rounding to float32
All take the float32 input as it is.  The inputs of the GPU tests are built here too.
"""

import functools

import numpy as np

RUN, SEGMENT = 33, 8192


def zero_state(sos):
    return np.zeros((len(sos), 2))


def truth(sos, x, state=None):
    """(y float64 [n], new state float64 [S][2]) of one row."""
    u = np.asarray(x, np.float32).astype(np.float64).tolist()
    state = zero_state(sos) if state is None else np.array(state, np.float64)
    for s, (b0, b1, b2, _, a1, a2) in enumerate(np.asarray(sos, np.float64).tolist()):
        z0, z1 = state[s].tolist()
        out = []
        push = out.append
        for v in u:
            y = b0 * v + z0
            z0 = b1 * v - a1 * y + z1
            z1 = b2 * v - a2 * y
            push(y)
        u = out
        state[s] = z0, z1
    return np.array(u, np.float64), state


def yardstick(sos, x, state=None):
    """(y float32 [rows][n], new state float32 [rows][S][2]) of rows x [rows][n]: every product and sum rounded to float32."""
    f = np.float32
    u = np.array(x, f, ndmin=2)
    rows, n = u.shape
    c = np.asarray(sos, np.float64).astype(f)
    state = np.zeros((rows, len(c), 2), f) if state is None else np.array(state, f)
    for s in range(len(c)):
        b0, b1, b2, _, a1, a2 = c[s]
        z0, z1 = state[:, s, 0].copy(), state[:, s, 1].copy()
        y = np.empty_like(u)
        for i in range(n):
            v = u[:, i]
            yi = b0 * v + z0
            z0 = b1 * v - a1 * yi + z1
            z1 = b2 * v - a2 * yi
            y[:, i] = yi
        u = y
        state[:, s, 0], state[:, s, 1] = z0, z1
    return u, state


def _sweep(c, u, cnt, z0, z1):
    """The recurrence over runs u [T][RUN] (run t has cnt[t] samples) from states z0, z1 [T]: (y [T][RUN], z0, z1)."""
    b0, b1, b2, _, a1, a2 = c
    y = np.zeros_like(u)
    z0, z1 = z0.copy(), z1.copy()
    for i in range(u.shape[1]):
        on = i < cnt
        yi = b0 * u[:, i] + z0
        n0 = b1 * u[:, i] - a1 * yi + z1
        n1 = b2 * u[:, i] - a2 * yi
        y[:, i] = np.where(on, yi, 0.0)
        z0, z1 = np.where(on, n0, z0), np.where(on, n1, z1)
    return y, z0, z1


def block(sos, x, state=None, run=RUN, segment=SEGMENT, dtype=np.float32):
    """(y float32 [n], new state float64 [S][2]) of one row, in the kernel's block form, all of it in float64 (dtype=np.float64:
    without the output's one rounding)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    sos = np.asarray(sos, np.float64)
    state = zero_state(sos) if state is None else np.array(state, np.float64)
    out = np.empty(len(x), dtype)
    for g0 in range(0, len(x), segment):
        seg = x[g0:g0 + segment]
        T = -(-len(seg) // run)
        u = np.zeros((T, run))
        u.reshape(-1)[:len(seg)] = seg
        cnt = np.minimum(run, len(seg) - run * np.arange(T))
        for s, c in enumerate(sos):
            M = np.array([[-c[4], 1.0], [-c[5], 0.0]])
            MR = np.linalg.matrix_power(M, run)
            _, v0, v1 = _sweep(c, u, cnt, np.zeros(T), np.zeros(T))
            enter = np.zeros((T, 2))
            enter[0] = state[s]
            for t in range(1, T):                            # every run before run t is whole
                enter[t] = MR @ enter[t - 1] + (v0[t - 1], v1[t - 1])
            u, z0, z1 = _sweep(c, u, cnt, enter[:, 0], enter[:, 1])
            state[s] = z0[-1], z1[-1]                        # the last non-empty run's
        out[g0:g0 + len(seg)] = u.reshape(-1)[:len(seg)].astype(dtype)
    return out, state


def audio_error(got, want):
    """max |got - want| relative to the row's output peak (of want)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    peak = float(np.max(np.abs(want))) if want.size else 0.0
    return float(np.max(np.abs(got - want))) / (peak if peak > 0 else 1.0) if want.size else 0.0


def state_error(got, want):
    """max |got - want| relative to the largest entry of the row's own state."""
    return audio_error(np.ravel(got), np.ravel(want))


def bound(yard):
    """What the GPU may differ from truth by, given the yardstick's own error on that row (the AGC test's rule)."""
    return min(max(4.0 * yard, 1e-6), 1e-4)


FLOOR = bound(0.0)          # no yardstick makes the bound smaller than this: an error below it needs none


# ---- inputs ----------------------------------------------------------------------------------------------------------

AMPLITUDES = (1.0, 0.03, 0.001)          # three rows over three decades
SIZES = (1, 2, 33, 255, 1000, 1001, 8000, 8192, 8193, 48000, 100003)


def rate_of(n):
    """The audio rate the filters of the primitive tests are designed for: the row lengths below one second of 8 kHz audio
    are pieces of such audio (a 300 Hz corner has no design at a rate of 255)."""
    return 48000 if n >= 48000 else 8000


def rows(n, call, rate=None, seed=0):
    """float32 [3][n], call `call` of consecutive calls of n samples: noise on a DC level of 0.5; an 88.5 Hz tone of 0.2
    under noise of 1; voice-band noise -- at AMPLITUDES."""
    rate = rate_of(n) if rate is None else rate
    rng = np.random.default_rng(1000 * seed + call)
    k = np.arange(call * n, (call + 1) * n)
    r0 = 0.5 + 0.3 * rng.standard_normal(n)
    r1 = 0.2 * np.sin(2 * np.pi * 88.5 * k / rate) + rng.standard_normal(n)
    r2 = np.convolve(rng.standard_normal(n + 7), np.ones(8) / np.sqrt(8.0), mode="valid")
    return (np.stack([r0, r1, r2]) * np.array(AMPLITUDES)[:, None]).astype(np.float32)


def stereo(x):
    """[3][n] -> [3][n][2]: the right leg of row r is row r + 1 (mod 3) at half the level.  A factor of two is exact in
    every float format, so the right leg's truth is the left leg's of that row, halved -- the model runs once for both."""
    return np.ascontiguousarray(np.stack([x, 0.5 * np.roll(x, -1, axis=0)], axis=2))


def stereo_of(a):
    """What stereo() makes of the inputs, made of the model's per-row results a [3][...]: [3][2][...]."""
    return np.stack([a, 0.5 * np.roll(a, -1, axis=0)], axis=1)


def elliptic(rate):
    """The hard case: an 8-section elliptic high-pass at 300 Hz whose poles lie within 1e-3 of the unit circle."""
    import scipy.signal
    return np.ascontiguousarray(scipy.signal.ellip(16, 0.5, 60, 300.0, "highpass", output="sos", fs=rate), dtype=np.float64)


def filters(n):
    """{name: sos float64 [S][6]} of the primitive test at row length n."""
    from radiocore.tools import audiofilter as af
    rate = rate_of(n)
    out = {"deemphasis": af.AudioFilter.deemphasis(750e-6).sections(rate), "highpass": af.AudioFilter.highpass(300.0).sections(rate)}
    if n >= 8000:
        out["voice_nfm"] = af.VOICE_NFM.sections(rate)
    if n in (8000, 48000):
        out["elliptic"] = elliptic(rate)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, n, calls=2):
    """Per call of rows(n, call) through filters(n)[name], the state carried from zero: {"x" [calls][3][n], "sos",
    "audio" (truth) [calls][3][n], "state" (truth) [calls][3][S][2]}, read-only."""
    sos = filters(n)[name]
    x = np.stack([rows(n, c) for c in range(calls)])
    audio = np.zeros(x.shape)
    state = np.zeros((calls, 3, len(sos), 2))
    for r in range(3):
        st = None
        for c in range(calls):
            audio[c, r], st = truth(sos, x[c, r], st)
            state[c, r] = st
    for a in (x, audio, state):
        a.setflags(write=False)
    return {"x": x, "sos": sos, "audio": audio, "state": state}


def yard_errors(name, n, call):
    """The yardstick's own errors on reference(name, n), call `call`: (audio [3], state [3]).  Costly: the GPU tests ask
    only where an error is above FLOOR."""
    ref = reference(name, n)
    st = None
    for c in range(call + 1):
        y, st = yardstick(ref["sos"], ref["x"][c], st)
    return (np.array([audio_error(y[r], ref["audio"][call, r]) for r in range(3)]),
            np.array([state_error(st[r], ref["state"][call, r]) for r in range(3)]))
