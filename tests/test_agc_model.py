"""CPU: the AGC model the GPU tests compare against (tests/agc_model.py) -- its three statements agree, the state
carries, the -1 start rule, the floor's gain cap -- and the yardstick's own error on every case the GPU tests use."""

import numpy as np
import pytest

import agc_model as m
import radiocore_oracle as oracle

MODES = [m.PEAK, m.CARRIER]
IDS = ["PEAK", "CARRIER"]


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("decay", [40.0, 2400.0, 14400.0])
def test_sequential_and_closed_form_agree(mode, decay):
    v = m.voice(6000, 5, mode) * 0.3
    for s in (-1.0, 0.0, 0.05, 2.0):
        a, sa = m.truth(v, mode, decay, 0.25, 1e-4, s)
        b, sb = m.closed(v, mode, decay, 0.25, 1e-4, s)
        assert np.max(np.abs(a - b)) <= 1e-12 and abs(sa - sb) <= 1e-12 * max(abs(sa), 1e-30), (decay, s)


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_one_row_equals_two_half_rows_with_the_state_carried(mode):
    v = m.voice(2000, 9, mode)
    for s in (-1.0, 0.4):
        if mode == m.CARRIER and s < 0:
            continue            # without history CARRIER starts from the mean of the CALL's row: the halves differ by design
        whole, sw = m.truth(v, mode, 700.0, 0.25, 1e-3, s)
        a, s1 = m.truth(v[:1000], mode, 700.0, 0.25, 1e-3, s)
        b, s2 = m.truth(v[1000:], mode, 700.0, 0.25, 1e-3, s1)
        assert np.max(np.abs(np.concatenate([a, b]) - whole)) <= 1e-12
        assert abs(s2 - sw) <= 1e-12 * abs(sw)


def test_start_rule():
    v = np.array([0.5, -0.25, 0.1], np.float32)
    lam = np.exp(-1.0 / 10.0)
    a, s = m.truth(v, m.PEAK, 10.0, 0.25, 0.0, -1.0)           # PEAK without history: e[-1] = 0
    e = [0.5, 0.5 * lam, 0.5 * lam * lam]
    assert np.allclose(a, 0.25 * v / e, rtol=1e-15) and abs(s - e[-1]) < 1e-15
    a0, s0 = m.truth(v, m.PEAK, 10.0, 0.25, 0.0, 0.0)          # ... and history 0 is the same thing
    assert np.array_equal(a, a0) and s == s0
    a1, _ = m.truth(v, m.PEAK, 10.0, 0.25, 0.0, 4.0)           # a large history holds the gain down
    assert np.allclose(a1, 0.25 * v / (4.0 * lam ** np.arange(1, 4)), rtol=1e-14)
    w = np.array([1.0, 1.2, 0.8, 1.0], np.float32)
    _, sc = m.truth(w, m.CARRIER, 10.0, 1.0, 0.0, -1.0)        # CARRIER without history: c[-1] = mean(v) of this call
    c = float(np.mean(w.astype(np.float64)))
    for x in w.astype(np.float64):
        c += (1 - lam) * (x - c)
    assert abs(sc - c) < 1e-15
    _, sneg = m.truth(w, m.CARRIER, 10.0, 1.0, 0.0, -0.5)      # any negative state means "no history"
    assert sneg == sc


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_floor_caps_the_gain(mode):
    """An empty channel (1e-6 of the floor) comes out at level / floor times its input, not at full scale; zeros give zeros."""
    rng = np.random.default_rng(3)
    v = (1e-6 * (1.0 + 0.1 * rng.standard_normal(500))).astype(np.float32)
    a, _ = m.truth(v, mode, 100.0, 0.25, 1.0, -1.0)
    assert np.max(np.abs(a)) <= (0.25 / 1.0) * 2.0 * float(np.max(np.abs(v)))        # gain <= level / floor
    free, _ = m.truth(v, mode, 100.0, 0.25, 0.0, -1.0)
    assert np.max(np.abs(free)) > (0.2 if mode == m.PEAK else 0.02)
    z, s = m.truth(np.zeros(50, np.float32), mode, 100.0, 0.25, 0.0, -1.0)
    assert not z.any() and s == 0.0


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("case", m.CASES)
def test_yardstick_error_on_the_primitive_cases(case, mode):
    """The float32 restatement stays within YARDSTICK_LIMIT of the row's peak on every primitive case of
    tests/test_hip_agc.py: four times it is then a bound that means something."""
    worst = 0.0
    for n in m.SIZES:
        ref = m.reference(case, mode, n)
        ya = ref["yard_audio"][~np.isnan(ref["yard_audio"])]
        print(case, IDS[mode], n, "yardstick audio %.3g state %.3g" % (ya.max(), np.nanmax(ref["yard_state"])))
        worst = max(worst, float(ya.max()))
    assert worst <= m.YARDSTICK_LIMIT, worst


@pytest.mark.parametrize("kind", ["AM", "USB", "LSB"])
@pytest.mark.parametrize("B,A", m.CHAIN_SIZES)
def test_yardstick_error_on_the_demodulator_cases(kind, B, A):
    vs = [m.chain_signal(oracle, kind, m.chain_iq(kind, B, buf), B, A) for buf in range(3)]
    floor = m.chain_floor(vs)
    assert all(floor >= 0.1 * np.max(np.abs(v)) for v in vs)        # level / floor does not amplify the chain's own 2e-6
    settings = m.chain_settings(kind, A, floor)
    want, _ = m.follow(vs, m.chain_mode(kind), settings)
    got, _ = m.follow(vs, m.chain_mode(kind), settings, m.yardstick)
    errs = [m.audio_error(g, w) for g, w in zip(got, want)]
    print(kind, B, A, "floor %.3g" % floor, "yardstick", ["%.3g" % e for e in errs])
    assert max(errs) <= m.YARDSTICK_LIMIT, errs
