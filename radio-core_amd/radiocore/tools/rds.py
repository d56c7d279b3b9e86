"""RDS on the host (IEC 62106), from the 57 kHz subcarrier tap of a WBFM channel to station identity: numpy only, no
device calls.  ``Tuner.subcarrier(Subcarrier(B, R, 57000, rds.taps(B, R)))`` gives every station's RDS baseband at R
complex samples per second (9 600 is plenty); per station

    station(groups(bits(y, R)))  ->  (PI code, 8-character programme service name)

There is no error correction: a block counts only when its syndrome is zero, a group only when all four blocks do.
No reference counterpart.
"""

import numpy as np

__all__ = ["taps", "bits", "groups", "station", "CHIP_RATE", "POLY", "OFFSETS"]

CHIP_RATE = 2375                     # two biphase chips per bit of 1187.5 bit/s
POLY = 0x5B9                         # g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}
_BLOCK_OFFSETS = ((OFFSETS["A"],), (OFFSETS["B"],), (OFFSETS["C"], OFFSETS["C'"]), (OFFSETS["D"],))
TIMING_STEPS = 16


def taps(input_size, output_size, ntaps=241, cutoff=3000.0):
    """Hamming windowed-sinc low-pass for a Subcarrier(input_size, output_size, ...): `ntaps` (odd) float32 taps, -6 dB at
    `cutoff` Hz of the input rate, unit DC gain.  The cutoff must lie below the output's Nyquist frequency."""
    B, R, T = int(input_size), int(output_size), int(ntaps)
    if T < 1 or T % 2 == 0:
        raise ValueError("the number of taps must be odd")
    if not 0.0 < float(cutoff) < 0.5 * R:
        raise ValueError("the cutoff must lie between 0 and half the output rate")
    m = np.arange(T) - 0.5 * (T - 1)
    h = np.sinc(2.0 * float(cutoff) / B * m)
    if T > 1:
        h = h * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(T) / (T - 1)))
    return (h / np.sum(h)).astype(np.float32)


def bits(y, rate):
    """Data bits (uint8) of one tap output y, `rate` complex samples per second.  Carrier phase 0.5 arg sum(y^2) (the
    sign it leaves open falls out of the differential decoding); chips at CHIP_RATE by linear interpolation, at the best
    of 16 timing offsets and 2 chip pairings by sum |c0 - c1|; bit = c0 > c1, then b[k] = e[k] ^ e[k - 1]."""
    y = np.asarray(y).astype(np.complex128).reshape(-1)
    if len(y) < 2:
        return np.zeros(0, np.uint8)
    phase = 0.5 * np.angle(np.sum(y * y))
    z = np.real(y * np.exp(-1j * phase))
    per_chip = float(rate) / CHIP_RATE
    pos = np.arange(len(z), dtype=np.float64)
    best, best_metric = None, -1.0
    for step in range(TIMING_STEPS):
        t = (np.arange(int((len(z) - 1) / per_chip) + 1) + step / TIMING_STEPS) * per_chip
        c = np.interp(t[t <= len(z) - 1], pos, z)
        for pair in (0, 1):
            n = (len(c) - pair) // 2
            c0, c1 = c[pair:pair + 2 * n:2], c[pair + 1:pair + 2 * n:2]
            metric = float(np.sum(np.abs(c0 - c1)))
            if metric > best_metric:
                best, best_metric = c0 > c1, metric
    e = best.astype(np.uint8)
    return e[1:] ^ e[:-1]


def _syndrome(block):
    """Remainder of a 26-bit word modulo g(x)."""
    for shift in range(25, 9, -1):
        if block >> shift & 1:
            block ^= POLY << (shift - 10)
    return block


def checkword(info, offset):
    """The 10 check bits of a 16-bit information word under an offset word."""
    return _syndrome(int(info) << 10) ^ offset


def groups(bits):
    """[(A, B, C, D)]: the 16-bit information words of every 104-bit group found sliding bit by bit through `bits`, accepted
    when all four 26-bit blocks have zero syndrome once their offset word (A, B, C or C', D) is removed."""
    b = np.asarray(bits).astype(np.int64).reshape(-1)
    if len(b) < 104:
        return []
    weights = 1 << np.arange(25, -1, -1, dtype=np.int64)
    # word[k] = the 26 bits that start at k, first bit most significant
    word = np.convolve(b, weights[::-1].astype(np.float64)).astype(np.int64)[25:len(b)]
    found, k = [], 0
    while k + 104 <= len(b):
        blocks = [int(word[k + 26 * i]) for i in range(4)]
        if all(any(_syndrome(blk ^ off) == 0 for off in offs) for blk, offs in zip(blocks, _BLOCK_OFFSETS)):
            found.append(tuple(blk >> 10 for blk in blocks))
            k += 104
        else:
            k += 1
    return found


def station(groups):
    """(PI, PS): the programme identification code (the most frequent block A; None without groups) and the 8-character
    programme service name from the type-0 groups -- segment = low two bits of block B, two characters from block D --
    with '?' where no segment arrived."""
    groups = list(groups)
    if not groups:
        return None, "?" * 8
    values, counts = np.unique([g[0] for g in groups], return_counts=True)
    pi = int(values[np.argmax(counts)])
    ps = ["?"] * 8
    for a, blk_b, _, d in groups:
        if a == pi and blk_b >> 12 == 0:
            seg = blk_b & 3
            ps[2 * seg], ps[2 * seg + 1] = chr(d >> 8), chr(d & 0xFF)
    return pi, "".join(ps)
