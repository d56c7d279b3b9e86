"""The audio filter's model (tests/sos_model.py) and radiocore.AudioFilter's designs, without a device: the truth against
scipy.signal.sosfilt, the block form against the truth, the designs against scipy.signal.butter, and every refusal of
the Python layer."""

import numpy as np
import pytest
import scipy.signal

import sos_model as m
from radiocore.tools import audiofilter as af
from radiocore.tools.audiofilter import AudioFilter


def _response(sos, rate, points=512):
    return scipy.signal.sosfreqz(sos, worN=points, fs=rate)


def test_truth_is_sosfilt_with_zi_carried():
    for name, n in (("highpass", 1000), ("voice_nfm", 8000), ("elliptic", 8000)):
        sos = m.filters(n)[name]
        zi = np.zeros((len(sos), 2))
        st = None
        for call in range(2):
            x = m.rows(n, call)[0]
            want, zi = scipy.signal.sosfilt(np.array(sos), x.astype(np.float64), zi=zi)
            got, st = m.truth(sos, x, st)
            assert m.audio_error(got, want) <= 1e-12, (name, call)
            assert m.state_error(st, zi) <= 1e-12, (name, call)


@pytest.mark.parametrize("n", [1, 33, 34, 8192, 8193, 20000])
def test_block_form_is_the_truth(n):
    """Runs of 33, the scan with M^R, segments of 8192, two calls with the state carried: 1e-9 of the peak before the
    output's one rounding to float32, which costs 6e-8 more."""
    for name in ("highpass", "elliptic"):
        sos = m.filters(8000)[name]
        st_t = st_b = st_prev = None
        for call in range(2):
            x = m.rows(n, call, rate=8000)[1]
            want, st_t = m.truth(sos, x, st_t)
            got, st_b = m.block(sos, x, st_b)
            assert got.dtype == np.float32
            assert m.state_error(st_b, st_t) <= 1e-9, (name, call)
            assert m.audio_error(got, want.astype(np.float32)) <= 1.2e-7, (name, call)
            exact, _ = m.block(sos, x, st_prev, dtype=np.float64)
            assert m.audio_error(exact, want) <= 1e-9, (name, call)
            st_prev = st_b.copy()


def test_yardstick_is_float32_and_close():
    sos = m.filters(8000)["highpass"]
    x = m.rows(2000, 0, rate=8000)
    y, st = m.yardstick(sos, x)
    assert y.dtype == np.float32 and st.dtype == np.float32 and y.shape == x.shape
    for r in range(3):
        want, s_want = m.truth(sos, x[r])
        e = m.audio_error(y[r], want)
        assert 1e-9 < e <= 1e-4, e                           # float32 costs something, and not much
    assert m.bound(0.0) == 1e-6 == m.FLOOR and m.bound(1.0) == 1e-4 and m.bound(5e-6) == 2e-5


def test_stereo_legs_are_exact_copies_of_rows():
    x = m.rows(50, 0)
    s = m.stereo(x)
    assert s.shape == (3, 50, 2) and s.dtype == np.float32
    assert np.array_equal(s[:, :, 0], x) and np.array_equal(s[0, :, 1], 0.5 * x[1]) and np.array_equal(s[2, :, 1], 0.5 * x[0])
    sos = m.filters(8000)["highpass"]
    assert np.array_equal(m.truth(sos, s[0, :, 1])[0], 0.5 * m.truth(sos, x[1])[0])
    assert np.array_equal(m.stereo_of(x)[0, 1], s[0, :, 1])


@pytest.mark.parametrize("A", [8000, 48000])
def test_designs_match_scipy_butter(A):
    cases = [(AudioFilter.highpass(300.0), scipy.signal.butter(4, 300.0, "highpass", output="sos", fs=A)),
             (AudioFilter.lowpass(3000.0), scipy.signal.butter(4, 3000.0, "lowpass", output="sos", fs=A)),
             (AudioFilter.highpass(250.0, order=5), scipy.signal.butter(5, 250.0, "highpass", output="sos", fs=A)),
             (AudioFilter.lowpass(3400.0, order=3), scipy.signal.butter(3, 3400.0, "lowpass", output="sos", fs=A)),
             (AudioFilter.lowpass(2500.0, order=1), scipy.signal.butter(1, 2500.0, "lowpass", output="sos", fs=A)),
             (AudioFilter.bandpass(300.0, 3400.0), scipy.signal.butter(4, [300.0, 3400.0], "bandpass", output="sos", fs=A)),
             (AudioFilter.bandpass(300.0, 3000.0, order=3), scipy.signal.butter(3, [300.0, 3000.0], "bandpass", output="sos", fs=A))]
    for filt, want in cases:
        got = filt.sections(A)
        assert got.dtype == np.float64 and got.shape == (len(filt), 6) == want.shape
        assert (got[:, 3] == 1.0).all()
        _, h_got = _response(got, A)
        _, h_want = _response(want, A)
        assert np.max(np.abs(h_got - h_want)) <= 1e-10, np.max(np.abs(h_got - h_want))
    both = AudioFilter.highpass(300.0) + AudioFilter.lowpass(3000.0)
    assert len(both) == 4
    assert np.array_equal(both.sections(A), np.concatenate([cases[0][0].sections(A), cases[1][0].sections(A)]))
    assert both.sections(A) is both.sections(A)


def _gain_db(sos, rate, f):
    _, h = scipy.signal.sosfreqz(sos, worN=np.atleast_1d(np.asarray(f, np.float64)), fs=rate)
    return 20 * np.log10(np.abs(h))


@pytest.mark.parametrize("A", [8000, 48000])
def test_deemphasis_corner_and_dc_gain(A):
    sos = AudioFilter.deemphasis(750e-6).sections(A)
    assert sos.shape == (1, 6) and sos[0, 2] == 0.0 and sos[0, 5] == 0.0
    assert abs(sos[0, :3].sum() / sos[0, 3:].sum() - 1.0) <= 1e-14             # H(z = 1)
    assert abs(_gain_db(sos, A, 212.0)[0] + 3.0103) <= 0.05
    assert _gain_db(sos, A, 2120.0)[0] < -19.0                                  # 6 dB per octave from there on


def test_voice_filters():
    nfm = af.VOICE_NFM.sections(8000)
    de = AudioFilter.deemphasis(750e-6).sections(8000)
    assert len(af.VOICE_NFM) == 5 and len(af.VOICE_AM) == 4
    assert _gain_db(nfm, 8000, 88.5)[0] - _gain_db(de, 8000, 88.5)[0] <= -30.0
    f = np.linspace(500.0, 2500.0, 81)
    assert np.max(np.abs(_gain_db(nfm, 8000, f) - _gain_db(de, 8000, f))) <= 1.0
    am = af.VOICE_AM.sections(8000)
    assert np.max(np.abs(_gain_db(am, 8000, np.linspace(600.0, 2800.0, 23)))) <= 1.0
    assert _gain_db(am, 8000, 100.0)[0] <= -30.0


def test_python_refusals():
    good = scipy.signal.butter(2, 300.0, "highpass", output="sos", fs=8000)
    # a corner at or above A / 2 (sections at that rate), for every constructor
    for filt in (AudioFilter.highpass(300.0), AudioFilter.lowpass(300.0), AudioFilter.bandpass(100.0, 300.0),
                 AudioFilter.deemphasis(1.0 / (2 * np.pi * 300.0))):
        for A in (600, 599, 100):
            with pytest.raises(ValueError):
                filt.sections(A)
        assert filt.sections(8000).shape[1] == 6
    for bad in (dict(f_hz=0.0), dict(f_hz=-5.0), dict(f_hz=float("nan"))):
        with pytest.raises(ValueError):
            AudioFilter.highpass(**bad).sections(8000)
    for order in (0, 17, 2.5):
        with pytest.raises(ValueError):
            AudioFilter.lowpass(300.0, order=order)
    with pytest.raises(ValueError):
        AudioFilter.bandpass(3000.0, 300.0)
    for tau in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError):
            AudioFilter.deemphasis(tau)
    # sos: unstable, not finite, a0 != 1, the wrong shape, too many sections, another rate
    for col, value in ((5, 1.0), (5, -1.0), (5, 1.5), (4, 2.5), (4, -2.5), (0, float("nan")), (1, float("inf")), (3, 2.0)):
        bad = good.copy()
        bad[0, col] = value
        with pytest.raises(ValueError):
            AudioFilter.sos(bad, 8000)
    for bad in (np.ones(6), np.ones((2, 5)), np.zeros((0, 6)), np.tile(good, (9, 1))):
        with pytest.raises(ValueError):
            AudioFilter.sos(bad, 8000)
    for rate in (0, -8000, 8000.5):
        with pytest.raises(ValueError):
            AudioFilter.sos(good, rate)
    ok = AudioFilter.sos(good, 8000)
    assert np.array_equal(ok.sections(8000), good)
    for A in (48000, 7999):
        with pytest.raises(ValueError):
            ok.sections(A)
    # more than 8 sections
    eight = AudioFilter.highpass(300.0, order=8) + AudioFilter.lowpass(3000.0, order=8)
    assert len(eight) == 8
    with pytest.raises(ValueError):
        eight + AudioFilter.deemphasis(750e-6)
    with pytest.raises(ValueError):
        AudioFilter.bandpass(300.0, 3000.0, order=9)
    with pytest.raises(ValueError):
        AudioFilter([])
    with pytest.raises(TypeError):
        ok + 3
