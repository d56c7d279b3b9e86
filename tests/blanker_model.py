"""The noise blanker's definition (include/rcfm.h, "noise blanker") in numpy, and the seeded inputs the blanker's tests share.

Samples are complex64 [n], or interleaved integers [n, 2] whose dtype names the format (int16, int8, uint8), as
``Tuner.load_raw`` takes them.  ``blank`` returns everything the definition names; nothing here touches a device."""

from types import SimpleNamespace

import numpy as np

MEDIAN, ABSOLUTE = 0, 1
FAR = 1 << 62          # "infinite" distance
FORMATS = {"cf32": np.dtype("complex64"), "cs16": np.dtype("int16"), "cs8": np.dtype("int8"), "cu8": np.dtype("uint8")}


def components(x):
    """(re, im) float32 [n] of a buffer: complex64 as it is, integers by the exact rules of rcfm_tuner_load_raw."""
    x = np.asarray(x)
    if x.dtype == np.complex64:
        v = x.view(np.float32).reshape(-1, 2)
        return v[:, 0].copy(), v[:, 1].copy()
    f = x.reshape(-1, 2).astype(np.float32)
    if x.dtype == np.int16:
        f *= np.float32(2.0 ** -15)
    elif x.dtype == np.int8:
        f *= np.float32(2.0 ** -7)
    elif x.dtype == np.uint8:
        f = (f - np.float32(127.5)) * np.float32(2.0 ** -7)
    else:
        raise ValueError("complex64, int16, int8 or uint8, not %s" % x.dtype)
    return f[:, 0].copy(), f[:, 1].copy()


def power(re, im):
    """p = fl32(fl32(re re) + fl32(im im)): three float32 operations, each rounded on its own."""
    with np.errstate(all="ignore"):
        return (re * re).astype(np.float32) + (im * im).astype(np.float32)


def block_means(re, im, L):
    """m [nb] float64: the pairwise tree over each block's L slots (zeros at and beyond n), divided by the block's own
    sample count; a non-finite mean counts as +inf."""
    n = re.shape[0]
    nb = -(-n // L)
    v = np.zeros(nb * L, np.float64)
    with np.errstate(all="ignore"):
        v[:n] = re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2
        v = v.reshape(nb, L)
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
        cnt = np.minimum(L, n - L * np.arange(nb)).astype(np.float64)
        m = v[:, 0] / cnt
    m[~np.isfinite(m)] = np.inf
    return m


def thresholds(m, span, mode, value):
    """t [nb] float32: (float)(value x lower median of m over the blocks within `span`), or (float)value in absolute mode."""
    nb = m.shape[0]
    with np.errstate(all="ignore"):
        if mode == ABSOLUTE:
            return np.full(nb, np.float32(value), np.float32)
        r = np.empty(nb, np.float64)
        for b in range(nb):
            w = np.sort(m[max(0, b - span):min(nb - 1, b + span) + 1])
            r[b] = w[(w.shape[0] - 1) // 2]
        return (np.float64(value) * r).astype(np.float32)


def distances(hit):
    """d [n] int64: the distance to the nearest hit, no wrap at the ends; FAR (beyond every gain table) where there is none."""
    n = hit.shape[0]
    idx = np.flatnonzero(hit)
    if idx.size == 0:
        return np.full(n, FAR, np.int64)
    i = np.arange(n)
    k = np.searchsorted(idx, i)
    right = np.where(k < idx.size, idx[np.minimum(k, idx.size - 1)] - i, FAR)
    left = np.where(k > 0, i - idx[np.maximum(k - 1, 0)], FAR)
    return np.minimum(left, right).astype(np.int64)


def gains(d, hold, ramp):
    """g [n] float32: 0 up to `hold`, the ramp table behind it, 1 beyond hold + len(ramp)."""
    ramp = np.asarray(ramp, np.float32).reshape(-1)
    G = hold + ramp.shape[0]
    g = np.ones(d.shape[0], np.float32)
    g[d <= hold] = 0.0
    on = (d > hold) & (d <= G)
    g[on] = ramp[d[on] - hold - 1]
    return g


def output(x, g):
    """The blanked buffer in x's own format: bit copies where g == 1, the format's zero where g == 0, scaled otherwise."""
    x = np.asarray(x)
    n = g.shape[0]
    one, zero = g == 1.0, g == 0.0
    i = np.arange(n)
    with np.errstate(all="ignore"):
        if x.dtype == np.complex64:
            v = x.view(np.float32).reshape(-1, 2)
            y = (g[:, None] * v).astype(np.float32)
            y[zero] = 0.0
            out = np.where(one[:, None], v.view(np.uint32), y.view(np.uint32))       # bits: NaN payloads and -0 survive
            return out.view(np.float32).reshape(-1).view(np.complex64)
        shape = x.shape
        v = x.reshape(-1, 2)
        f = v.astype(np.float32)
        if x.dtype == np.uint8:
            y = np.rint(np.float32(127.5) + (g[:, None] * (f - np.float32(127.5))).astype(np.float32)).astype(np.int64)
            y[zero] = (127 + (i[zero] & 1))[:, None]
        else:
            y = np.rint((g[:, None] * f).astype(np.float32)).astype(np.int64)
            y[zero] = 0
        return np.where(one[:, None], v, y.astype(x.dtype)).reshape(shape)


def blank(x, block=4096, span=4, mode=MEDIAN, value=10.0 ** 1.2, hold=0, ramp=()):
    """Everything the definition names, for one buffer: m, t, p, hit, d, g, out and stats = (hits, samples with g < 1)."""
    re, im = components(x)
    p = power(re, im)
    m = block_means(re, im, block)
    t = thresholds(m, span, mode, value)
    with np.errstate(all="ignore"):
        hit = p > t[np.arange(p.shape[0]) // block]
    d = distances(hit)
    g = gains(d, hold, ramp)
    return SimpleNamespace(p=p, m=m, t=t, hit=hit, d=d, g=g, out=output(x, g),
                           stats=(int(hit.sum()), int((g < 1.0).sum())))


def robust(x, block=4096, span=4, mode=MEDIAN, value=10.0 ** 1.2, **_):
    """True when no sample's p lies within 2^-22 t of its block's threshold: a threshold one float32 ulp (2^-23 t at most)
    away from the model's then decides every hit as the model does."""
    re, im = components(x)
    p = power(re, im).astype(np.float64)
    t = thresholds(block_means(re, im, block), span, mode, value).astype(np.float64)
    tb = t[np.arange(p.shape[0]) // block]
    ok = np.isfinite(tb) & np.isfinite(p)
    return bool(np.all(np.abs(p[ok] - tb[ok]) > 2.0 ** -22 * tb[ok]))


def mask_words(hit):
    """The hit bitmask as the device leaves it: bit i & 31 of word i >> 5, whole tiles of 4096 samples."""
    n = hit.shape[0]
    bits = np.zeros(-(-n // 4096) * 4096, np.uint8)
    bits[:n] = hit
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def raised_cosine(R):
    """The ramp NoiseBlanker builds: 0.5 (1 - cos(pi (j + 1) / (R + 1))), j = 0 .. R - 1, in float64, rounded to float32."""
    j = np.arange(R, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(np.pi * (j + 1.0) / (R + 1.0)))).astype(np.float32)


# ---- the seeded inputs of tests/test_blanker_model.py and tests/test_hip_blanker.py -------------------------------------

_SIGMA = {"cf32": 0.05, "cs16": 0.008, "cs8": 0.03, "cu8": 0.03}      # per component; pulses sit at full scale
_PEAK = {"cf32": (4.0, -3.0), "cs16": (-32768, 32767), "cs8": (-128, 127), "cu8": (255, 0)}
SHAPES = (1, 63, 64, 65, 1000, 4096, 4097, 12289, 100003)
BLOCKS = (64, 256, 4096)
SPANS = (0, 1, 4, 8)
GUARDS = ((0, 0), (0, 5), (8, 8), (1000, 24))
RATIO = 10.0 ** 1.2            # 12 dB over the median


def pulse_positions(n, block, guard, stretch=False):
    """Where the tests plant pulses: both ends, the tile edge, a block edge, two closer than the guard; stretch: 5000 in a row."""
    pos = {0, n - 1, 4095, 4096, block - 1, block, 3 * block + 7, 3 * block + 7 + max(guard // 2, 1), n // 2}
    if stretch:
        pos |= set(range(5000, 10000))
    return np.array(sorted(q for q in pos if 0 <= q < n), np.int64)


def make_input(fmt, n, seed, positions=()):
    """Noise with full-scale pulses at `positions`, in format `fmt`: complex64 [n] or integers [n, 2]."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 2)) * _SIGMA[fmt]
    pos = np.asarray(positions, np.int64)
    if fmt == "cf32":
        x = z.astype(np.float32)
        x[pos] = _PEAK[fmt]
        x[pos[1::2]] *= -1.0
        return x.reshape(-1).view(np.complex64)
    dt = FORMATS[fmt]
    if fmt == "cs16":
        x = np.clip(np.rint(z * 32768.0), -32768, 32767)
    elif fmt == "cs8":
        x = np.clip(np.rint(z * 128.0), -128, 127)
    else:
        x = np.clip(np.rint(z * 128.0 + 127.5), 0, 255)
    x = x.astype(dt)
    x[pos] = _PEAK[fmt]
    x[pos[1::2]] = _PEAK[fmt][::-1]
    return x


def absolute_level(fmt):
    """A threshold for RCFM_BLANK_ABSOLUTE between the noise of `make_input` and its pulses (the power of a sample)."""
    return 400.0 * 2.0 * _SIGMA[fmt] ** 2


def shape_cases():
    """(fmt, n, block, span, hold, ramp length, mode, seed) for every shape, block and span, the formats, guards and modes
    taken in turn -- each of them meets every n."""
    fmts = list(FORMATS)
    cases = []
    k = 0
    for n in SHAPES:
        for block in BLOCKS:
            for span in SPANS:
                fmt = fmts[k % 4]
                hold, R = GUARDS[(k // 4 + k) % 4]
                mode = ABSOLUTE if k % 5 == 4 else MEDIAN
                cases.append((fmt, n, block, span, hold, R, mode, 1000 + k))
                k += 1
    return cases


def case_input(case, stretch=False):
    fmt, n, block, span, hold, R, mode, seed = case
    x = make_input(fmt, n, seed, pulse_positions(n, block, hold + R, stretch))
    kw = dict(block=block, span=span, mode=mode, value=absolute_level(fmt) if mode == ABSOLUTE else RATIO, hold=hold,
              ramp=raised_cosine(R))
    return x, kw
