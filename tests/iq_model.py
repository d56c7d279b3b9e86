"""Raw integer IQ (include/rcfm.h, RCFM_IQ_*) in numpy: the three conversions as the header states them, in float32, and
seeded full-range buffers with the extreme values planted where a kernel's first and last lanes and its second tile line
read them."""

import numpy as np

RCFM_IQ_CS16, RCFM_IQ_CS8, RCFM_IQ_CU8 = 1, 2, 3
DTYPES = {RCFM_IQ_CS16: np.dtype("int16"), RCFM_IQ_CS8: np.dtype("int8"), RCFM_IQ_CU8: np.dtype("uint8")}
NAMES = {RCFM_IQ_CS16: "cs16", RCFM_IQ_CS8: "cs8", RCFM_IQ_CU8: "cu8"}


def to_float32(values):
    """float32 of integer samples of one of the three types: i * 2^-15, i * 2^-7, (u - 127.5) * 2^-7."""
    v = np.asarray(values)
    f = v.astype(np.float32)
    if v.dtype == np.int16:
        return f * np.float32(2.0 ** -15)
    if v.dtype == np.int8:
        return f * np.float32(2.0 ** -7)
    if v.dtype == np.uint8:
        return (f - np.float32(127.5)) * np.float32(2.0 ** -7)
    raise ValueError("raw IQ is int16, int8 or uint8, not %s" % v.dtype)


def to_complex64(raw):
    """complex64 [N] of interleaved I, Q integers shaped [N, 2] or [2 N]."""
    f = to_float32(np.asarray(raw).reshape(-1, 2))
    return np.ascontiguousarray(f).view(np.complex64).reshape(-1)


def exact_float64(values):
    """What the conversion means, in float64: i / 32768, i / 128, (u - 127.5) / 128."""
    v = np.asarray(values)
    d = v.astype(np.float64)
    return {np.dtype("int16"): d / 32768.0, np.dtype("int8"): d / 128.0, np.dtype("uint8"): (d - 127.5) / 128.0}[v.dtype]


def all_values(dtype):
    info = np.iinfo(dtype)
    return np.arange(info.min, info.max + 1, dtype=np.int64).astype(dtype)


def random_pairs(fmt, n, seed, line=None):
    """[n, 2] uniform over the type's full range; the extremes (min, max / max, min) at samples 0, 1, n - 1 and, when given,
    at sample `line`: the first element of the second tile line of the transform's first pass."""
    dt = DTYPES[fmt]
    info = np.iinfo(dt)
    r = np.random.default_rng(seed)
    x = r.integers(info.min, info.max + 1, size=(n, 2), dtype=np.int64).astype(dt)
    spots = [0, 1, n - 1] + ([line] if line is not None and 0 <= line < n else [])
    for k, s in enumerate(spots):
        if s < n:
            x[s] = (info.min, info.max) if k % 2 == 0 else (info.max, info.min)
    return x
