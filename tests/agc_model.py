"""AGC test model (no test functions): the stateful AGC of include/rcfm.h (rcfm_agc / rcfm_demod_set_agc) in numpy.

    lambda = exp(-1 / decay_samples), alpha = 1 - lambda
    PEAK     e[n] = max(|v[n]|, lambda e[n-1]), e[-1] = s;   audio = clip(level v / max(e, floor), +-0.999)
    CARRIER  c[n] = c[n-1] + alpha (v[n] - c[n-1]), c[-1] = s;  audio = clip(level (v - c) / max(c, floor), +-0.999)
    audio = 0 where the denominator is not > 0; s < 0: PEAK starts from 0, CARRIER from mean(v); the new s is the
    follower after the last sample.

Three statements of it:
    truth       float64, sample after sample
    closed      float64, closed form (running maximum / running sum in a decaying frame): must agree with truth
    yardstick   float32, sample after sample, in the forms a float32 receiver would use -- e - alpha e and
                c + alpha (v - c), each as one fused multiply-add.  Its distance from truth is what float32 costs; the
                GPU tests allow four times that (within 1e-6 .. 1e-4).
All take the float32 input as it is.  The inputs of the GPU tests are built here too, so that the CPU tests can check
the yardstick on exactly those.
"""

import functools
import struct

import numpy as np

PEAK, CARRIER = 0, 1            # RCFM_AGC_PEAK, RCFM_AGC_CARRIER
CLIP = 0.999
YARDSTICK_LIMIT = 2.5e-5        # the yardstick's own error on every case the GPU tests use (tests/test_agc_model.py)

_F32 = struct.Struct("f")


def _r32(y):
    """A Python float rounded to float32 (once)."""
    return _F32.unpack(_F32.pack(y))[0]


def alpha_of(decay_samples):
    return -np.expm1(-1.0 / float(decay_samples))


def _start(v, mode, s):
    if s < 0:
        return 0.0 if mode == PEAK else float(np.mean(v.astype(np.float64)))
    return float(s)


def _divide(v, follower, mode, level, floor):
    den = np.maximum(follower, floor)
    num = level * (v if mode == PEAK else v - follower)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, np.clip(num / den, -CLIP, CLIP), 0.0)


def truth(v, mode, decay_samples, level, floor, s=-1.0):
    """(audio float64 [n], new state float64): the definition, sample after sample in float64."""
    v = np.asarray(v, np.float32).astype(np.float64)
    a = alpha_of(decay_samples)
    lam = 1.0 - a
    f = _start(v, mode, s)
    out = []
    if mode == PEAK:
        for x in np.abs(v).tolist():
            f = lam * f
            if x > f:
                f = x
            out.append(f)
    else:
        for x in v.tolist():
            f = f + a * (x - f)
            out.append(f)
    fol = np.array(out)
    return _divide(v, fol, mode, level, floor), f


def closed(v, mode, decay_samples, level, floor, s=-1.0):
    """The same in closed form (finite input, n / decay_samples < 600).  In the frame that grows by exp(1 / decay) per sample
    the peak follower is a running maximum and the carrier follower a running sum."""
    v = np.asarray(v, np.float32).astype(np.float64)
    n, d = len(v), float(decay_samples)
    assert n / d < 600
    k = np.arange(n)
    f0 = _start(v, mode, s)
    if mode == PEAK:
        with np.errstate(divide="ignore"):
            lg = np.log(np.abs(v)) + k / d
            top = np.maximum(np.maximum.accumulate(lg), (np.log(f0) - 1.0 / d) if f0 > 0 else -np.inf)   # s lambda^(n + 1)
        fol = np.exp(top - k / d)
    else:
        a = alpha_of(d)
        fol = np.exp(-k / d) * ((1.0 - a) * f0 + a * np.cumsum(v * np.exp(k / d)))
    return _divide(v, fol, mode, level, floor), float(fol[-1])


def yardstick(v, mode, decay_samples, level, floor, s=-1.0):
    """(audio float32 [n], new state float32): float32 sample after sample, the alpha forms with one rounding each."""
    v32 = np.asarray(v, np.float32)
    a = _r32(alpha_of(decay_samples))
    f = _r32(_start(v32, mode, s))
    out = []
    if mode == PEAK:
        for x in np.abs(v32).tolist():
            f = _r32(f - a * f)                 # the product of two float32 is exact in float64: one rounding, as an fma
            if x > f:
                f = x
            out.append(f)
    else:
        for x in v32.tolist():
            f = _r32(f + a * _r32(x - f))
            out.append(f)
    fol = np.array(out, np.float32)
    den = np.maximum(fol, np.float32(floor))
    num = np.float32(level) * (v32 if mode == PEAK else v32 - fol)
    with np.errstate(divide="ignore", invalid="ignore"):
        audio = np.where(den > 0, np.clip(num / den, np.float32(-CLIP), np.float32(CLIP)), np.float32(0))
    return audio.astype(np.float32), np.float32(f)


def audio_error(got, want):
    """max |got - want| relative to the row's peak (of want); exact zeros are wanted where want is all zero."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    peak = float(np.max(np.abs(want))) if len(want) else 0.0
    return float(np.max(np.abs(got - want))) / (peak if peak > 0 else 1.0)


def state_error(got, want):
    return abs(float(got) - float(want)) / (abs(float(want)) if want != 0 else 1.0)


def bound(yard):
    """What the GPU may differ from truth by, given the yardstick's own error on that row."""
    return min(max(4.0 * yard, 1e-6), 1e-4)


# ---- inputs ----------------------------------------------------------------------------------------------------------

AMPLITUDES = (1.0, 0.03, 0.001)          # C = 3 rows over three decades
SIZES = (1, 255, 1000, 1001, 8000, 48000, 100003)


def decay_for(n):
    """0.3 s of 8 kHz audio, whatever the row's length (the long rows are long recordings): the float32 carrier follower of
    the yardstick loses accuracy with the square root of decay_samples and would leave its limit at 0.3 s of 48 kHz."""
    return 0.3 * 8000


def voice(n, seed, mode):
    """Voice-like bursts, float32 [n] of peak about 1: band-limited noise under a syllable envelope with pauses; for CARRIER
    a carrier of 1 modulated by it at 50 %, over white noise of 5 % of the carrier."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n + 8)
    x = np.convolve(x, np.ones(8) / np.sqrt(8.0), mode="valid")[:n]              # low-pass: neighbouring samples cohere
    t = np.arange(n) / 8000.0
    env = np.clip(np.sin(2 * np.pi * (3.1 * t + rng.uniform())) * 1.5, 0.0, 1.0)  # ~3 syllables a second, pauses between
    s = 0.3 * x * env
    if mode == CARRIER:
        # A float32 one-pole follower stops moving once alpha |v - c| falls below half an ulp of c: |v - c| < 9e-4 c at
        # alpha = 7e-5.  A carrier that is exactly constant through a pause would park the yardstick there, 30 times
        # outside its limit; real carriers come with noise, which keeps it moving.
        return (1.0 + 0.5 * np.clip(s, -1, 1) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return s.astype(np.float32)


def rows(case, mode, n):
    """The C = 3 rows of a primitive case, float32 [calls][3][n], with its (decay_samples, level, floor)."""
    level = 0.25 if mode == PEAK else 1.0
    amps = np.array(AMPLITUDES)[:, None]
    if case == "voice":
        calls = [np.stack([voice(n, 10 * c + r + 1, mode) for r in range(3)]) * amps for c in range(2)]
        return np.array(calls, np.float32), (decay_for(n), level, 1e-5)
    if case == "peak_then_quiet":       # one peak, then 1e-9 of it for two whole calls; decay_samples = 2 n, the state carried
        # floor: 0, so that the audio shows the follower's whole decay -- except for PEAK at n = 100 003, where the float32
        # yardstick itself drifts 6.2e-5 over the two calls (2.5 times its limit): that size raises the floor to 0.8 of
        # the largest row's peak, and the rest of the decay is checked through the state
        a = np.full((2, 3, n), 1e-9)
        a[0, :, min(3, n - 1)] = 1.0
        floor = 0.8 * amps[:, 0].max() if (mode == PEAK and n > 48000) else 0.0
        return (a * amps).astype(np.float32), (2.0 * n, level, floor)
    if case == "zeros":
        return np.zeros((2, 3, n), np.float32), (decay_for(n), level, 0.0)
    if case == "nan_row":               # a NaN in the middle row, between two clean rows
        a = np.array([np.stack([voice(n, 50 + r, mode) for r in range(3)]) * amps for c in range(2)])
        a[0, 1, n // 2] = np.nan
        return a.astype(np.float32), (decay_for(n), level, 1e-5)
    raise KeyError(case)


CASES = ("voice", "peak_then_quiet", "zeros", "nan_row")


@functools.lru_cache(maxsize=None)
def reference(case, mode, n):
    """Per call and row of rows(case, mode, n), the state carried from call to call and starting at -1:
    {"v", "params", "audio" (truth), "state" (truth), "yard_audio", "yard_state": the yardstick's own errors}.
    Rows with a NaN are followed by the yardstick only up to None."""
    v, (decay, level, floor) = rows(case, mode, n)
    calls, C = v.shape[0], v.shape[1]
    audio = np.zeros(v.shape)
    state = np.zeros((calls, C))
    ya = np.zeros((calls, C))
    ys = np.zeros((calls, C))
    for r in range(C):
        s_t, s_y = -1.0, -1.0
        for c in range(calls):
            if np.isnan(v[:c + 1, r]).any():
                audio[c, r], state[c, r], ya[c, r], ys[c, r] = np.nan, np.nan, np.nan, np.nan
                continue
            audio[c, r], s_t = truth(v[c, r], mode, decay, level, floor, s_t)
            y, s_y = yardstick(v[c, r], mode, decay, level, floor, s_y)
            state[c, r] = s_t
            ya[c, r] = audio_error(y, audio[c, r])
            ys[c, r] = state_error(s_y, s_t)
    for a in (v, audio, state, ya, ys):
        a.setflags(write=False)
    return {"v": v, "params": (decay, level, floor), "audio": audio, "state": state, "yard_audio": ya, "yard_state": ys}


# ---- the demodulators with agc -----------------------------------------------------------------------------------------

CHAIN_SIZES = ((25000, 8000), (3001, 1000))       # (B, A); prime B: rocFFT, no DC bin
CHAIN_STEPS = (0.05, 0.5, 0.05)                   # station level of three consecutive buffers: x10 and back
CHAIN_DECAY = 0.3                                 # seconds


def chain_iq(kind, B, buf):
    """complex64 [B]: the station of buffer `buf` (AM: am_model.station, USB / LSB: ssb_model.station) at CHAIN_STEPS[buf]."""
    import am_model
    import ssb_model
    if kind == "AM":
        x = am_model.station(2, B, seed=40 + buf, level=CHAIN_STEPS[buf])
    else:
        x = ssb_model.station(2, B, seed=40 + buf, level=CHAIN_STEPS[buf])
    return x.astype(np.complex64)


def chain_signal(oracle, kind, iq, B, A):
    """v: what the AGC tail of a demodulator sees, float64 [A]: AM's decimated envelope, the decimated sideband of USB / LSB."""
    import ssb_model
    if kind == "AM":
        e = np.abs(np.asarray(iq).astype(np.complex64)).astype(np.float32)
        return np.asarray(oracle.Decimate(B, A).run(e), np.float64)
    return ssb_model.sideband(oracle, iq, B, A, kind == "LSB")


def chain_mode(kind):
    return CARRIER if kind == "AM" else PEAK


def chain_settings(kind, A, floor):
    """(decay_samples, level, floor) of radiocore.AGC(decay=CHAIN_DECAY, floor=floor) on this class."""
    return CHAIN_DECAY * A, (1.0 if kind == "AM" else 0.25), floor


def chain_floor(vs):
    """A floor of 0.1 of the largest buffer's peak, so >= 0.1 of every row's: level / floor does not amplify the chain's own 2e-6."""
    return 0.1 * max(float(np.max(np.abs(v))) for v in vs)


def follow(vs, mode, settings, fn=truth):
    """[audio] of consecutive buffers vs through `fn` (truth / yardstick), the state carried from -1, and the last state."""
    s, out = -1.0, []
    for v in vs:
        a, s = fn(np.asarray(v, np.float32), mode, *settings, s)
        out.append(a)
    return out, s
