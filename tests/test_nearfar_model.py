"""The near-far model (tests/nearfar_model.py) without a GPU: the inputs of tests/test_hip_nearfar.py are well
conditioned row by row, the float32 emulation of the pair routes loses a weak row next to a strong one (so the device
tests have teeth), and the truth taken from a wideband spectrum is a float64 evaluation of the model the other AM / SSB
tests use.

Bounds: TOL (tests/conftest.py) and 0.1 TOL, the suite's bound for a reference against the float64 truth.
"""

import functools

import numpy as np
import pytest

import agc_model
import am_model
import nearfar_model as nf
import radiocore_oracle as oracle
import signal_edges as se
import ssb_model
from conftest import TOL, rel_err


@functools.lru_cache(maxsize=None)
def _unit(kind, B, A):
    rows = nf.unit_rows(kind, B, A)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _truth(kind, B, A):
    out = np.stack([nf.expect64(kind, x, B, A) for x in _unit(kind, B, A)])
    out.setflags(write=False)
    return out


def test_pattern_is_exact_in_float32():
    for kind, B, A in nf.GEOMETRIES:
        unit = _unit(kind, B, A)
        for k in nf.LEVELS_K:
            p = nf.pattern(k)
            assert p.tolist() == [1.0, 2.0 ** -k, 2.0 ** -k, 1.0, 2.0 ** -k]
            rows = nf.scaled(unit, k)
            assert rows.dtype == np.complex64
            back = rows.astype(np.complex128) / p[:, None]
            assert np.array_equal(back, unit.astype(np.complex128)), (kind, B, k)


@pytest.mark.parametrize("kind,B,A", nf.GEOMETRIES)
def test_every_row_is_well_conditioned_by_itself(kind, B, A):
    """The oracle's own float32 evaluation of each row ALONE, at every level, against the float64 one of the level-1
    row: 0.1 TOL.  A weak row is not ill conditioned by itself, and the scale drops out exactly."""
    truth = _truth(kind, B, A)
    worst = 0.0
    for k in nf.LEVELS_K:
        rows = nf.scaled(_unit(kind, B, A), k)
        for i in range(nf.BATCH):
            e = rel_err(nf.expect32(kind, rows[i], B, A), truth[i])
            worst = max(worst, e)
            assert e <= 0.1 * TOL, (kind, B, A, k, i, e)
            assert rel_err(nf.expect64(kind, rows[i], B, A), truth[i]) <= 1e-12, (k, i)
    print(kind, B, A, "float32 alone, worst over levels and rows: %.2e" % worst)


@pytest.mark.parametrize("kind,B,A", nf.GEOMETRIES)
def test_pair_emulation_in_float64_is_the_model(kind, B, A):
    """paired() with complex128 transforms is the expectation: the packing and unpacking themselves are exact."""
    got = nf.paired(kind, nf.scaled(_unit(kind, B, A), 13), B, A, np.complex128)
    for i in range(nf.BATCH):
        assert rel_err(got[i], _truth(kind, B, A)[i]) <= 1e-9, (kind, i)


@pytest.mark.parametrize("kind,B,A", [nf.AM_ENGINE, ("USB",) + nf.SSB_ENGINE])
def test_pair_emulation_has_teeth(kind, B, A):
    """The float32 pair route in numpy: the weak member of a pair leaves TOL when its partner is 78 dB stronger, stays
    inside it up to 42 dB, and neither the strong rows nor the lone last row notice anything at any level."""
    truth = _truth(kind, B, A)
    table = {}
    for k in nf.LEVELS_K:
        got = nf.paired_float32(kind, nf.scaled(_unit(kind, B, A), k), B, A)
        table[k] = [rel_err(got[i], truth[i]) for i in range(nf.BATCH)]
        print(kind, "k = %2d (%2.0f dB):" % (k, 6.0206 * k), " ".join("%.2e" % e for e in table[k]))
    for i in nf.WEAK:
        if i != nf.LONE:
            assert table[13][i] > TOL, (kind, i, table[13])
    for k in (0, 7):
        assert max(table[k]) <= TOL, (kind, k, table[k])
    for k in nf.LEVELS_K:
        for i in nf.STRONG + (nf.LONE,):
            assert table[k][i] <= 0.1 * TOL, (kind, k, i, table[k])


@pytest.mark.parametrize("kind,B,A", [nf.AM_ENGINE, ("USB",) + nf.SSB_ENGINE])
def test_agc_case_is_well_conditioned(kind, B, A):
    """The AGC case of the device test, row by row and alone: the oracle's float32 signal through agc_model.truth against
    the float64 signal through it, audio and state within 0.1 TOL at both levels -- the floor of the weak level does not
    turn the strong rows' rounding into an audible error."""
    units, vs, settings = nf.agc_case(kind, B, A)
    mode = agc_model.chain_mode(kind)
    p = nf.pattern(nf.AGC_K)
    for i in range(nf.BATCH):
        want, s_want = agc_model.follow([vs[buf][i] * p[i] for buf in range(nf.AGC_BUFFERS)], mode, settings)
        v32 = [nf.signal32(kind, nf.scaled(units[buf], nf.AGC_K)[i], B, A) for buf in range(nf.AGC_BUFFERS)]
        got, s_got = agc_model.follow(v32, mode, settings)
        ea = max(rel_err(got[buf], want[buf]) for buf in range(nf.AGC_BUFFERS))
        es = agc_model.state_error(s_got, s_want)
        print(kind, "row", i, "level %.3g: audio %.2e state %.2e" % (p[i], ea, es))
        assert ea <= 0.1 * TOL and es <= 0.1 * TOL, (kind, i, ea, es)
        _, s_unit = agc_model.follow([vs[buf][i] for buf in range(nf.AGC_BUFFERS)], mode, settings)
        assert abs(s_want - s_unit * p[i]) <= 1e-12 * s_unit * p[i]      # the state does not see the floor: it scales


PIPELINE = {"AM": (1_000_000, 25000, 8000), "USB": (1_000_000, 12500, 8000), "LSB": (1_000_000, 12500, 8000)}


@pytest.mark.parametrize("kind", list(PIPELINE))
def test_from_spectrum_is_the_model_in_float64(kind):
    """On an oracle Tuner's own spectrum from_spectrum gives what am_model / ssb_model.expect_channel give from that
    Tuner's channel samples -- in float64, whatever precision the spectrum was computed in."""
    N, B, A = PIPELINE[kind]
    C = nf.BATCH
    ref = se.oracle_tuner(B, C, N)
    x = se.wideband_from(list(nf.unit_rows(kind, B, A)), N, ref.input_frequency, se.centres_of(B, C), B,
                         gain=0.3 * nf.pattern(10), noise=0.0)
    ref.load(x.astype(np.complex128))
    X = ref._buffer
    assert X.dtype == np.complex128
    for i in range(C):
        roll, m = ref._roll(i)
        got = nf.from_spectrum(oracle, X, N, roll, m, A, kind)
        assert got.dtype == np.float64 and got.shape == (A, 1)
        want = (am_model.expect_channel(oracle, ref, i, A) if kind == "AM"
                else ssb_model.expect_channel(oracle, ref, i, A, kind == "LSB"))
        e = rel_err(got, want)
        print(kind, "channel", i, "from_spectrum against expect_channel: %.2e" % e)
        assert e <= 1e-6, (kind, i, e)
