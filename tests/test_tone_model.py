"""CPU: the tone bank's definition (tests/tone_model.py, the float64 model the GPU tests compare against) has the
properties include/rcfm.h states, the float32 yardstick agrees with it, and the host side of the detection
(radiocore.tools.tones) reads tones and SELCAL codes out of its results."""

import numpy as np
import pytest

import tone_model
from radiocore.tools import tones


def test_a_sinusoid_at_a_tone_gives_a_squared_over_four():
    """Exactly at nu[k], amplitude a: P = a^2 / 4 for the rect and the Hann window alike (the window's sum normalises),
    and E = a^2 / 2."""
    A, a = 8000, 0.3
    freqs = np.array([100.0, 250.0, 1000.0])
    x = np.stack([tone_model.tone(A, f, a, phase=0.7 * i) for i, f in enumerate(freqs)]).astype(np.float32)
    for window in (None, tone_model.hann(A)):
        P, E = tone_model.tone_bank(x, freqs / A, A, window)
        assert P.shape == (3, 1, 3) and E.shape == (3, 1)
        for c in range(3):
            assert abs(P[c, 0, c] - a * a / 4) <= 1e-6 * a * a, (c, P[c, 0])
            assert np.all(np.delete(P[c, 0], c) <= 1e-9)            # whole cycles apart: the other tones see nothing
        assert np.allclose(E, a * a / 2, rtol=1e-6)
    # frames: 100 Hz in frames of 800 samples is ten whole cycles
    P, E = tone_model.tone_bank(x[:1], freqs[:1] / A, 800, tone_model.hann(800))
    assert P.shape == (1, 10, 1) and np.allclose(P, a * a / 4, rtol=1e-5)


def test_the_tail_is_ignored_and_the_phase_is_frame_local():
    rng = np.random.default_rng(1)
    A, L = 1000, 160
    nu = np.array([0.013, 0.1234, 0.5])
    x = rng.standard_normal((2, A)).astype(np.float32)
    w = rng.uniform(0.1, 1.0, L).astype(np.float32)
    P, E = tone_model.tone_bank(x, nu, L, w)
    assert P.shape == (2, 6, 3) and E.shape == (2, 6)
    y = x.copy()
    y[:, 960:] = 1e6                                             # A mod L = 40 samples behind the last frame
    P2, E2 = tone_model.tone_bank(y, nu, L, w)
    assert np.array_equal(P, P2) and np.array_equal(E, E2)
    # frame-local phase: frame f of x is frame 0 of x shifted by f L samples, whatever nu L is
    for f in range(6):
        Pf, Ef = tone_model.tone_bank(x[:, f * L:(f + 1) * L], nu, L, w)
        assert np.allclose(Pf[:, 0], P[:, f], rtol=1e-12, atol=0) and np.allclose(Ef[:, 0], E[:, f], rtol=1e-12)
    with pytest.raises(ValueError):
        tone_model.tone_bank(x[:, :100], nu, L, w)


def test_step_and_offset_address_one_side_of_interleaved_stereo():
    rng = np.random.default_rng(2)
    A, L = 640, 320
    nu = np.array([0.01, 0.2])
    left, right = rng.standard_normal((2, 3, A)).astype(np.float32)
    stereo = np.stack([left, right], axis=2)                    # [C, A, 2], the byte layout of WBFM's audio
    for audio in (stereo, stereo.reshape(3, 2 * A)):
        for offset, side in ((0, left), (1, right)):
            got = tone_model.tone_bank(audio, nu, L, None, step=2, offset=offset)
            want = tone_model.tone_bank(side, nu, L, None)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    garbage = stereo.copy()
    garbage[:, :, 1] = np.nan
    assert np.array_equal(tone_model.tone_bank(garbage, nu, L, None, step=2)[0], tone_model.tone_bank(left, nu, L)[0])


def test_the_float32_yardstick_agrees_with_the_model():
    rng = np.random.default_rng(3)
    A, L = 1000, 160
    nu = np.array(tones.CTCSS) / 8000.0
    x = (0.2 * rng.standard_normal((2, A)) + 0.1 * np.cos(2 * np.pi * nu[5] * np.arange(A))).astype(np.float32)
    w = tone_model.hann(L)
    P, E = tone_model.tone_bank(x, nu, L, w)
    P32, E32 = tone_model.tone_bank_f32(x, nu, L, w)
    assert P32.dtype == np.float32 and E32.dtype == np.float32
    err = np.max(np.abs(P32 - P) / tone_model.largest_power(x, L, w)[..., None])
    assert 0 < err <= 2e-6, err
    assert np.max(np.abs(E32 - E) / E) <= 1e-6
    assert np.all(P <= tone_model.largest_power(x, L, w)[..., None] * (1 + 1e-12))


def test_tone_score_rules():
    P = np.zeros((5, 3, 4))
    E = np.ones((5, 3))
    P[0, :, 2] = (0.1, 0.4, 0.2)
    E[0] = (1.0, 2.0, 0.0)                                      # the E == 0 frame contributes 0, not inf
    P[1, :, 0] = (0.3, 0.3, 0.3)
    E[2] = 0.0                                                  # a silent channel: every frame contributes 0
    want = np.array([2, -1, 1, 0, 7])
    s = tone_model.tone_score(P, E, want)
    assert s[0] == 0.2 and s[1] == np.inf and s[2] == 0.0 and s[3] == 0.0 and np.isnan(s[4])
    gate = np.array([1, 0, 1, 1, 1], np.uint8)
    g = tone_model.tone_score(P, E, want, gate)
    assert g[0] == 0.2 and np.isnan(g[1]) and g[2] == 0.0        # gate == 0 wins over want == -1
    mask = tone_model.open_mask(g, 0.15)
    assert mask.tolist() == [True, False, False, False, False]   # NaN never opens
    assert tone_model.open_mask(s, 0.15).tolist() == [True, True, False, False, False]
    assert tone_model.margin(np.array([0.2, np.inf, 0.0, np.nan, 0.05]), 0.1) == 2.0


def test_strongest():
    P = np.zeros((2, 2, 5))
    E = np.ones((2, 2))
    P[0, 0] = (0.0, 0.3, 0.05, 0.2, 0.0)
    P[0, 1] = (0.001, 0.002, 0.0, 0.0, 0.0)
    P[1, 0] = (0.2, 0.2, 0.0, 0.0, 0.5)
    E[1, 1] = 0.0
    P[1, 1] = 1.0
    one = tones.strongest(P, E, 0.1)
    assert one.shape == (2, 2, 1) and one[..., 0].tolist() == [[1, -1], [4, -1]]
    two = tones.strongest(P, E, 0.1, n=2)
    assert two.tolist() == [[[1, 3], [-1, -1]], [[4, 0], [-1, -1]]]      # equal shares: the lower index first
    three = tones.strongest(P, E, 0.1, n=3)
    assert three[0, 0].tolist() == [1, 3, -1]
    with pytest.raises(ValueError):
        tones.strongest(P, E[:1], 0.1)
    with pytest.raises(ValueError):
        tones.strongest(P, E, 0.1, n=6)


def test_tables():
    assert len(tones.CTCSS) == 39 and tones.CTCSS[0] == 67.0 and tones.CTCSS[8] == 88.5 and tones.CTCSS[-1] == 250.3
    assert list(tones.CTCSS) == sorted(set(tones.CTCSS))
    assert len(tones.SELCAL) == 16 == len(tones.SELCAL_LETTERS) and tones.SELCAL_LETTERS == "ABCDEFGHJKLMPQRS"
    assert tones.SELCAL[0] == 312.6 and tones.SELCAL[-1] == 1479.1 and list(tones.SELCAL) == sorted(tones.SELCAL)


def test_selcal_code_over_three_buffers():
    """A synthetic call -- one second of tones A + M, 0.2 s of silence, one second of D + Q, in noise -- that starts in the
    middle of one buffer and ends in the third: frames of 2000 samples at 8 kHz, the strongest two tones of each frame
    strung together over the buffers."""
    A, L = 8000, 2000
    rng = np.random.default_rng(7)
    n = np.arange(3 * A)
    x = 0.02 * rng.standard_normal(3 * A)
    f = dict(zip(tones.SELCAL_LETTERS, tones.SELCAL))
    for letters, lo, hi in (("AM", 4000, 12000), ("DQ", 13600, 21600)):
        for ch in letters:
            x[lo:hi] += 0.2 * np.cos(2 * np.pi * f[ch] * n[lo:hi] / A)
    nu = np.array(tones.SELCAL) / A
    series = []
    for b in range(3):
        P, E = tone_model.tone_bank(x[None, b * A:(b + 1) * A].astype(np.float32), nu, L, tone_model.hann(L))
        series.extend(tones.strongest(P, E, 0.1, n=2)[0])
    assert len(series) == 12
    assert tones.selcal_code(series) == "AM-DQ"
    assert tones.selcal_code(series, min_frames=2) == "AM-DQ"
    assert tones.selcal_code(series[:6]) is None                 # the first pair alone is no call
    assert tones.selcal_code([(-1, -1)] * 5) is None
    assert tones.selcal_code([(11, 0), (0, 11), (-1, 3), (13, 3)]) == "AM-DQ"      # the order inside a pair does not matter


def test_every_ctcss_tone_stands_out_of_its_own_channel():
    """The separation the tone squelch relies on: A = L = 8000, Hann, a tone of amplitude 0.1 under Gaussian "speech" of
    sigma = 0.2 -- every one of the 39 tones is the strongest of its own channel, and ratio = 0.01 has at least 3x room
    on both sides in the model."""
    A, ratio = 8000, 0.01
    rng = np.random.default_rng(11)
    x = np.stack([tone_model.speech(rng, A) + tone_model.tone(A, f, 0.1, phase=rng.uniform(0, 6.28)) for f in tones.CTCSS])
    P, E = tone_model.tone_bank(x.astype(np.float32), np.array(tones.CTCSS) / A, A, tone_model.hann(A))
    share = P[:, 0, :] / E[:, 0, None]
    own = np.diag(share)
    other = share[~np.eye(39, dtype=bool)]
    print("own share >= %.4f, every other tone <= %.5f" % (own.min(), other.max()))
    assert np.array_equal(np.argmax(share, axis=1), np.arange(39))
    assert own.min() >= 3 * ratio and other.max() <= ratio / 3
    assert tones.strongest(P, E, ratio)[:, 0, 0].tolist() == list(range(39))
    want = np.arange(39)
    assert tone_model.open_mask(tone_model.tone_score(P, E, want), ratio).all()
    assert not tone_model.open_mask(tone_model.tone_score(P, E, (want + 1) % 39), ratio).any()
