"""An RDS encoder and a generator of RDS-carrying WBFM stations (no test functions; CPU only, numpy only).

Encoder (IEC 62106): 16-bit information words get the 10 check bits of g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 plus the
block's offset word; type-0A groups (PI | group type 0, TP, PTY, segment | two alternative-frequency codes | two PS
characters) cycle through the four segments of the 8-character programme service name; the bit stream is differentially
encoded, e[k] = b[k] ^ e[k - 1], and each e becomes two biphase chips (+1, -1 for a one, -1, +1 for a zero) at 2375 chips per
second, shaped with a raised cosine two chips wide (zero at the neighbouring chip centres).

Station: the multiplex
    mpx = 0.9 * 0.85 * (0.5 (l + r) + 0.5 (l - r) sin 2 th_p) + 0.09 sin th_p + 0.04 s(t) sin(3 th_p + 0.3),   th_p = 2 pi 19000 t,
frequency-modulates a carrier with 75 kHz peak deviation: exp(j 2 pi 75000 cumsum(mpx) / B), B samples of one second (the
multiplex is nudged by a constant below 2 / B so that the phase closes on itself at the buffer's end, as signal_edges does).
band() puts the stations on their centres in an N-sample buffer, band-limited (signal_edges.wideband_from), with noise.

None of this enters the product: radiocore.tools.rds is the decoder, written separately; its constants (polynomial,
offset words) are the standard's and are restated here on purpose.
"""

import functools

import numpy as np

import signal_edges

POLY = 0x5B9
OFFSET_A, OFFSET_B, OFFSET_C, OFFSET_D = 0x0FC, 0x198, 0x168, 0x1B4
CHIP_RATE = 2375
DEVIATION = 75000.0
RDS_LEVEL = 0.04
RDS_PHASE = 0.3

# the Tuner case of tests/subcarrier_model.py: N, B, centres relative to 100 MHz, amplitudes, noise, (PI, PS) per station
N, B = 2_400_000, 240_000
CENTRES = (100e6 - 700_000, 100e6 + 100_000, 100e6 + 850_000)
AMPLITUDES = (0.3, 0.1, 0.06)
NOISE = 1e-3
STATIONS = ((0xD314, "RADIO 1 "), (0x53C7, "KLASSIK*"), (0xA20F, " Jazz FM"))


def remainder(word):
    """word(x) mod g(x) for a word of up to 26 bits."""
    for shift in range(25, 9, -1):
        if word >> shift & 1:
            word ^= POLY << (shift - 10)
    return word


def block(info, offset):
    """26 bits, first bit first: the information word, then checkword + offset word."""
    word = (info << 10) | (remainder(info << 10) ^ offset)
    return [(word >> (25 - k)) & 1 for k in range(26)]


def group_0a(pi, ps, segment, pty=10, tp=1):
    """The 104 bits of one type-0A group carrying characters 2 segment, 2 segment + 1 of the 8-character name."""
    assert len(ps) == 8 and 0 <= segment < 4
    b = (0 << 12) | (0 << 11) | (tp << 10) | (pty << 5) | (1 << 3) | segment
    c = (0xE2 << 8) | (0x10 + segment)                      # two alternative-frequency codes
    d = (ord(ps[2 * segment]) << 8) | ord(ps[2 * segment + 1])
    return block(pi, OFFSET_A) + block(b, OFFSET_B) + block(c, OFFSET_C) + block(d, OFFSET_D)


def bit_stream(pi, ps, nbits, skip=0):
    """nbits data bits of the endless 0A stream of a station, starting `skip` bits into it."""
    out, seg = [], 0
    while len(out) < nbits + skip:
        out += group_0a(pi, ps, seg)
        seg = (seg + 1) % 4
    return np.array(out[skip:skip + nbits], np.uint8)


def chips(bits):
    """Differential encoding (the bit before the first is 0), then biphase: [2 len(bits)] of +-1."""
    e = np.bitwise_xor.accumulate(np.asarray(bits, np.uint8))
    s = 2.0 * e - 1.0
    return np.stack([s, -s], axis=1).reshape(-1)


def baseband(chip, rate, count, delay=0.0):
    """s(t) at t = n / rate, n = 0 .. count - 1: chip k is a raised cosine centred at (k + 1/2 + delay) / CHIP_RATE seconds,
    two chips wide.  (Chips before the first and beyond the last are zero.)"""
    u = np.arange(count, dtype=np.float64) * (CHIP_RATE / float(rate)) - 0.5 - delay
    k = np.floor(u).astype(np.int64)
    frac = u - k
    padded = np.concatenate([[0.0], np.asarray(chip, np.float64), [0.0, 0.0]])
    k = np.clip(k, -1, len(chip))
    return padded[k + 1] * 0.5 * (1.0 + np.cos(np.pi * frac)) + padded[k + 2] * 0.5 * (1.0 - np.cos(np.pi * frac))


def multiplex(i, size, pi, ps):
    """Station i's multiplex, [size] float64 in units of the peak deviation, and the data bits it carries."""
    rng = np.random.default_rng(5100 + i)
    t = np.arange(size, dtype=np.float64) / size
    left = sum(0.4 * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) for f in (440 + 31 * i, 2500 + 17 * i))
    right = sum(0.4 * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) for f in (660 + 13 * i, 5000 + 7 * i))
    bits = bit_stream(pi, ps, CHIP_RATE // 2 + 2, skip=17 + 29 * i)
    s = baseband(chips(bits), size, size, delay=0.13 + 0.21 * i)
    th = 2 * np.pi * 19000 * t
    mpx = 0.9 * 0.85 * (0.5 * (left + right) + 0.5 * (left - right) * np.sin(2 * th)) + 0.09 * np.sin(th) \
        + RDS_LEVEL * s * np.sin(3 * th + RDS_PHASE)
    return mpx, bits


def station_iq(i, size, pi, ps):
    """complex128 [size]: station i of one second at `size` samples per second."""
    mpx, _ = multiplex(i, size, pi, ps)
    step = 2.0 * DEVIATION / size * mpx                         # phase step / pi
    total = float(np.sum(step))
    step = step + (2.0 * np.round(total / 2.0) - total) / size   # the phase closes at the buffer's end
    return np.exp(1j * np.pi * np.cumsum(step))


def input_frequency():
    """radiocore.Tuner's arithmetic for CENTRES and bandwidth B (tuner.py:163-174): the middle of the occupied band."""
    return 0.5 * ((min(CENTRES) - B / 2) + (max(CENTRES) + B / 2))


@functools.lru_cache(maxsize=None)
def band():
    """complex64 [N]: the three stations on their centres plus complex noise; read-only, shared between tests."""
    st = [station_iq(i, B, pi, ps) for i, (pi, ps) in enumerate(STATIONS)]
    x = signal_edges.wideband_from(st, N, input_frequency(), CENTRES, B, gain=AMPLITUDES, noise=NOISE, seed=57)
    x.setflags(write=False)
    return x
