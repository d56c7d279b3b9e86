"""CPU: the carrier-estimate model (tests/carrier_model.py) against hand-computed cases, the conditions that keep the GPU
test's exact comparisons honest, the float32 yardstick behind its bounds, and the host side of retune: the roll
arithmetic, radiocore.tools.afc.corrections and the Tuner's fine-tune bookkeeping with the ABI replaced by a stand-in."""

import numpy as np
import pytest

import carrier_model as cm
from test_tuner_bookkeeping import FM, _FakeTensor, _tuner, fake_backend  # noqa: F401  (the fixture)


def _spectrum(n, tones):
    X = np.zeros(n, np.complex128)
    for s, a in tones:
        X[s % n] += a * n
    return X


# ---- the model against hand-computed cases ------------------------------------------------------------------------------

@pytest.mark.parametrize("n,B,s,d", [(1000, 100, 200, 17), (1000, 100, -300, -50), (1001, 101, 0, 50), (64, 64, 5, -32),
                                     (1000, 7, 499, 3)])
def test_pure_tone(n, B, s, d):
    """One tone at offset d of a channel centred on signed bin s (roll -s): peak_bin = d, peak_power = a^2, centroid = d,
    spread = 0 -- through the wrap of the element index too."""
    X = _spectrum(n, [(s + d, 0.5)])
    pb, pp, ce, sp = cm.carriers(X, n, [-s], [B], 0.0)
    assert pb[0] == d and pp[0] == pytest.approx(0.25, rel=1e-12)
    assert ce[0] == pytest.approx(d, abs=1e-9) and sp[0] == pytest.approx(0.0, abs=1e-4)
    dd, idx = cm.bins(n, -s, B)
    assert dd[0] == -(B // 2) and dd.size == B and idx[list(dd).index(d)] == (s + d) % n


def test_two_tones_centroid_and_spread():
    """Powers 1 and 4 at offsets -10 and 20: centroid (-10 + 80) / 5 = 14, variance (100 + 1600) / 5 - 196 = 144."""
    X = _spectrum(4096, [(700 - 10, 1.0), (700 + 20, 2.0)])
    pb, pp, ce, sp = cm.carriers(X, 4096, [-700], [200], 0.0)
    assert pb[0] == 20 and pp[0] == pytest.approx(4.0)
    assert ce[0] == pytest.approx(14.0) and sp[0] == pytest.approx(12.0)


def test_gate_includes_and_excludes():
    """A bin is gated in iff p_d >= G: exactly at the gate it is in, just below it is out; the peak ignores the gate."""
    n = 1024
    X = _spectrum(n, [(-5, 1.0), (7, 0.5), (30, 0.25)])           # powers 1, 0.25, 0.0625 (all exact in float32)
    run = lambda g: cm.carriers(X, n, [0], [100], g)
    assert run(0.0625)[2][0] == pytest.approx((-5 + 7 * 0.25 + 30 * 0.0625) / 1.3125)
    assert run(0.0626)[2][0] == pytest.approx((-5 + 7 * 0.25) / 1.25)
    assert run(0.25)[2][0] == pytest.approx((-5 + 7 * 0.25) / 1.25)
    assert run(0.5)[2][0] == pytest.approx(-5.0) and run(0.5)[3][0] == 0.0
    pb, pp, ce, sp = run(2.0)                                      # nothing gated in
    assert (pb[0], pp[0], ce[0], sp[0]) == (-5, 1.0, 0.0, 0.0)


def test_zero_power_and_ties_and_nan():
    n = 256
    pb, pp, ce, sp = cm.carriers(np.zeros(n, np.complex128), n, [3], [16], 0.0)
    assert (pb[0], pp[0], ce[0], sp[0]) == (-8, 0.0, 0.0, 0.0)    # S0 = 0: zeros; every bin ties: the lowest d
    X = _spectrum(n, [(4, 1.0), (-6, 1.0), (9, 1.0)])
    assert cm.carriers(X, n, [0], [32], 0.0)[0][0] == -6
    X[4] = np.nan
    pb, pp, _, _ = cm.carriers(X, n, [0], [32], 0.0)
    assert pb[0] == -6 and pp[0] == 1.0                            # a NaN never wins


# ---- the GPU inputs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cm.CASES))
def test_gpu_inputs_are_honest_and_the_yardstick_holds(name):
    """On every input of tests/test_hip_carriers.py, from the model alone: every channel's strongest bin leads the second
    strongest by >= 6 dB (no channel is left out of the exact peak_bin comparison), no bin lies within a factor
    1 +- 1e-3 of the gate, and the float32 yardstick stays below its pinned constants -- and finds the same peaks."""
    n, rolls, bws, x, X = cm.case(name)
    for gate in cm.GATES:
        lead, near = cm.honesty(X, n, rolls, bws, gate)
        exp = cm.expected(name, gate)
        got = cm.yardstick(x, n, rolls, bws, gate)
        cen, spr = float(np.max(np.abs(got[2] - exp[2]))), float(np.max(np.abs(got[3] - exp[3])))
        rel = float(np.max(np.abs(got[1] - exp[1]) / exp[1]))
        print("%s gate %g: %d channels, lead %.2f dB, nearest bin to the gate %.3g, float32 centroid %.3g spread %.3g bins, "
              "peak power %.3g relative" % (name, gate, len(bws), lead, near, cen, spr, rel))
        assert lead >= 6.0 and near >= 1e-3
        assert np.array_equal(got[0], exp[0])
        bound = cm.YARDSTICK[(name, gate > 0)]
        assert cen < bound[0] and spr < bound[1], (cen, spr, bound)
        assert bound[0] < 10 * cen and bound[1] < 10 * spr, "a pinned constant far above what it bounds"
        assert rel < cm.PEAK_POWER_REL / 4
        if gate > 0:                                               # the gate does something: it changes the estimates
            assert np.max(np.abs(exp[2] - cm.expected(name, 0.0)[2])) > 1.0


def test_fast_case_covers_what_it_claims():
    n, rolls, bws, _, _ = cm.case("fast")
    assert {25000, 12500, 2001, 7} == set(bws)
    for B in (25000, 12500, 2001, 7):
        assert {(-r) % 2 for r, b in zip(rolls, bws) if b == B} == {0, 1}          # even and odd base
    assert cm.segments(25000) == 4 and cm.segments(12500) == 2 and cm.segments(2001) == 1
    off = cm.boundary_offsets(25000, 1)
    assert off[0] == -12500 and off[-1] == 12499 and {-12500 + 8192 - 1, -12500 + 8192} <= set(off)


# ---- retune: arithmetic, afc.corrections, bookkeeping --------------------------------------------------------------------

def test_retune_moves_the_peak_to_zero():
    """bin d of a channel is X[(d - roll) mod n]: with roll - k instead of roll, what read d = k reads d = 0."""
    n, B, roll, k = 5000, 300, 1234, -77
    X = _spectrum(n, [(-roll + k, 1.0)])
    assert cm.carriers(X, n, [roll], [B], 0.0)[0][0] == k
    assert cm.carriers(X, n, [roll - k], [B], 0.0)[0][0] == 0
    assert cm.carriers(X, n, [(roll - k) % n - 3 * n], [B], 0.0)[0][0] == 0           # modulo n


def test_afc_corrections():
    from radiocore.tools import afc
    pb = np.array([10, -2000, 7, 0, 300], np.int32)
    pp = np.array([1.0, 2.0, 0.01, np.nan, 0.5], np.float32)
    ce = np.array([9.6, -1999.5, 7.4, 0.0, 310.49], np.float32)
    got = afc.corrections(pb, pp, ce, 0.1, 500)
    assert got.dtype == np.int64 and got.tolist() == [10, -500, 0, 0, 300]
    assert afc.corrections(pb, pp, ce, 0.1, 5000, use="centroid").tolist() == [10, -2000, 0, 0, 310]
    assert afc.corrections(pb, pp, ce, [2.0, 0.0, 0.0, 0.0, 1.0], 5000).tolist() == [0, -2000, 7, 0, 0]
    with pytest.raises(ValueError):
        afc.corrections(pb, pp, ce, 0.1, 500, use="median")
    with pytest.raises(ValueError):
        afc.corrections(pb, pp[:3], ce, 0.1, 500)
    import radiocore.tools
    assert radiocore.tools.corrections is afc.corrections


def test_tuner_retune_bookkeeping(fake_backend):
    """Cumulative, cleared by add_channel, geometry untouched; the handle is retuned, not rebuilt; a handle created
    later for the same channel list starts from the retuned rolls."""
    lib = fake_backend
    C = 6
    t = _tuner(C)
    N = 1_000_000
    t.request_bandwidth(float(N))
    geometry = (t.input_frequency, t.input_bandwidth, [c.center_frequency for c in t.channels()], t._version)
    base = list(t._rolls(None))
    assert t.fine_tune().tolist() == [0] * C
    t.retune(5)                                                    # no handle yet: nothing to call
    assert "rcfm_tuner_retune" not in lib.calls
    t.load(_FakeTensor((N,)))
    assert lib.calls["rcfm_tuner_create"] == 1 and "rcfm_tuner_retune" not in lib.calls     # created from the retuned rolls
    assert list(t._abi_arrays[1]) == [r - 5 for r in base]
    t.retune([1, -2, 0, 0, 0, 7])
    assert lib.calls["rcfm_tuner_retune"] == 1 and lib.calls["rcfm_tuner_create"] == 1
    assert t.fine_tune().tolist() == [6, 3, 5, 5, 5, 12]
    assert list(t._rolls(t._fine)) == [r - k for r, k in zip(base, [6, 3, 5, 5, 5, 12])]
    assert (t.input_frequency, t.input_bandwidth, [c.center_frequency for c in t.channels()], t._version) == geometry
    t.load(_FakeTensor((N,)))                                       # the steady state does not retune again
    assert lib.calls["rcfm_tuner_retune"] == 1
    t.fine_tune()[0] = 99                                           # a copy
    assert t.fine_tune()[0] == 6
    for bad in ([1, 2], 0.5, [[1] * C]):
        with pytest.raises(ValueError):
            t.retune(bad)
    t.retune(2.0)                                                   # an integer-valued float is a number of bins
    assert t.fine_tune().tolist() == [8, 5, 7, 7, 7, 14]
    # a lane follows the base tuner's fine-tune at its next load
    lane = t._lane_clone()
    lane.load(_FakeTensor((N,)))
    assert lib.calls["rcfm_tuner_create"] == 2 and list(lane._abi_arrays[1]) == list(t._rolls(t._fine))
    before = lib.calls["rcfm_tuner_retune"]
    t.retune(-1)
    lane._sync_lane(t)
    assert lib.calls["rcfm_tuner_retune"] == before + 1             # the base's own handle; the lane's waits for its load
    lane.load(_FakeTensor((N,)))
    assert lib.calls["rcfm_tuner_retune"] == before + 2 and lane.fine_tune().tolist() == t.fine_tune().tolist()
    t.add_channel(t.channels()[-1].center_frequency + 12000, 12500, FM(12500, 8000))
    assert t.fine_tune().tolist() == [0] * (C + 1)
