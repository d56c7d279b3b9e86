"""CPU: radiocore.tools.rds, the host-side RDS decoder, against the encoder and station generator of tests/rds_model.py:
the low-pass design, the round trip encode -> tap (float64 model) -> bits -> groups -> station, and what noise decodes to.
"""

import numpy as np
import pytest

import rds_model
import subcarrier_model as sm
from radiocore.tools import rds


def test_taps_are_a_unit_gain_symmetric_low_pass():
    h = rds.taps(240000, 9600)
    assert h.dtype == np.float32 and h.shape == (241,)
    assert abs(float(np.sum(h.astype(np.float64))) - 1.0) < 1e-6
    assert np.array_equal(h, h[::-1])
    H = np.abs(np.fft.rfft(h.astype(np.float64), 240000))
    assert abs(H[3000] - 0.5) < 0.01                 # -6 dB at the cutoff
    assert H[1000] > 0.95 and np.max(H[6600:]) < 0.01
    assert np.array_equal(h, sm.rds_taps(240000, 9600, 241, 3000.0))
    assert np.array_equal(rds.taps(1000, 100, 1, 20.0), np.ones(1, np.float32))
    for bad in (dict(ntaps=240), dict(cutoff=4800.0), dict(cutoff=0.0)):
        with pytest.raises(ValueError):
            rds.taps(240000, 9600, **bad)


def test_constants_are_the_standards():
    assert rds.POLY == rds_model.POLY == 0b10110111001
    assert (rds.OFFSETS["A"], rds.OFFSETS["B"], rds.OFFSETS["C"], rds.OFFSETS["C'"], rds.OFFSETS["D"]) == \
        (0x0FC, 0x198, 0x168, 0x350, 0x1B4)
    assert rds.CHIP_RATE == rds_model.CHIP_RATE == 2375
    for info in (0, 1, 0xD314, 0xFFFF):
        assert rds.checkword(info, rds.OFFSETS["B"]) == rds_model.remainder(info << 10) ^ rds_model.OFFSET_B


def test_groups_finds_every_group_of_a_clean_bit_stream():
    pi, ps = rds_model.STATIONS[0]
    b = rds_model.bit_stream(pi, ps, 104 * 9 + 80, skip=31)
    found = rds.groups(b)
    assert len(found) == 9                           # the first whole group starts 73 bits in
    assert rds.station(found) == (pi, ps)
    segs = [g[1] & 3 for g in found]
    assert segs == [(segs[0] + k) % 4 for k in range(9)]
    # block C' in place of C is accepted as well
    c_prime = rds_model.block(pi, rds_model.OFFSET_A) + rds_model.block(0x0800, rds_model.OFFSET_B) + \
        rds_model.block(pi, 0x350) + rds_model.block(0x4142, rds_model.OFFSET_D)
    assert rds.groups(c_prime) == [(pi, 0x0800, pi, 0x4142)]
    # one wrong bit: no group (syndrome-zero blocks only, no correction)
    c_prime[40] ^= 1
    assert rds.groups(c_prime) == []


def test_bits_undoes_the_chip_coding():
    """Chips at 9 600 samples per second, any timing, either carrier sign and phase: the data bits come back."""
    b = rds_model.bit_stream(0x1234, "ABCDEFGH", 600)
    for delay, phase in ((0.0, 0.0), (0.37, 2.0), (0.81, -1.1)):
        y = rds_model.baseband(rds_model.chips(b), 9600, 4800, delay) * np.exp(1j * phase)
        got = rds.bits(y, 9600)
        # the first decoded bit needs the chip pair before it: allow the stream to start one or two bits in
        assert any(np.array_equal(got[:500], b[k:k + 500]) for k in (1, 2)), (delay, phase)


def test_three_stations_round_trip_on_the_float64_model():
    R = sm.RDS_TAP[0]
    y = sm.rds_truth()
    for k, (pi, ps) in enumerate(rds_model.STATIONS):
        found = rds.groups(rds.bits(y[k], R))
        print("station %d: %d groups, %r" % (k, len(found), rds.station(found)))
        assert len(found) >= 8
        assert rds.station(found) == (pi, ps)
        sent = rds_model.multiplex(k, rds_model.B, pi, ps)[1]
        words = {tuple(int("".join(map(str, sent[s + 26 * i:s + 26 * i + 16])), 2) for i in range(4))
                 for s in range(len(sent) - 103)}
        assert set(found) <= words                   # every group found was sent


def test_noise_decodes_to_nothing():
    rng = np.random.default_rng(9)
    assert rds.groups(rng.integers(0, 2, 50000)) == []
    y = rng.standard_normal(9600) + 1j * rng.standard_normal(9600)
    found = rds.groups(rds.bits(y, 9600))
    assert found == [] and rds.station(found) == (None, "????????")
    assert rds.groups([]) == [] and len(rds.bits(np.zeros(0, np.complex64), 9600)) == 0
