"""CPU: the IQ balance model (tests/iqbal_model.py) -- the algebra of include/rcfm.h's "IQ balance" block, the index rules,
the band restriction, the quality of the blind estimate on every input the GPU tests load, and its documented failure --
and the host helpers of radiocore.tools.iq that share those definitions."""

import numpy as np
import pytest

import iqbal_model as model


def test_beta_inverts_c_exactly():
    rng = np.random.default_rng(1)
    for _ in range(200):
        beta = rng.uniform(0, 0.9) * np.exp(2j * np.pi * rng.uniform())       # (the inverse loses digits as |beta| -> 1)
        c = 2 * beta / (1 + abs(beta) ** 2)
        got = model.finish([c.real, c.imag, 2.0])            # P = c, Q = 2: c = 2 P / Q
        assert abs(got - beta) <= 1e-14, (beta, got)
    assert model.finish([0.3, 0.1, 0.0]) == 0 and model.finish([np.nan, 0.0, 1.0]) == 0 and model.finish([0.0, np.inf, 1.0]) == 0
    assert model.finish([1.0, 0.0, 2.0]) == 1.0              # |c| = 1: the square root's argument is clamped at 0


def test_true_beta_removes_the_image_exactly():
    rng = np.random.default_rng(2)
    for n in (3, 4, 16, 257):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        mu, nu, beta = model.receiver()
        X, Xi = np.fft.fft(x), np.fft.fft(model.impair(x))
        assert np.allclose(Xi, mu * X + nu * np.conj(X[model.mirror(n)]), rtol=0, atol=1e-12 * np.abs(X).max())
        Y = model.correct(Xi, beta)
        want = (mu - abs(nu) ** 2 / np.conj(mu)) * X
        assert np.max(np.abs(Y - want)) <= 1e-14 * np.abs(X).max() * n, n


def test_host_helpers_agree_with_the_model():
    from radiocore.tools import iq
    mu, nu, beta = iq.imbalance(model.GAIN, model.PHASE)
    assert (mu, nu, beta) == model.receiver()
    assert abs(20 * np.log10(abs(nu / mu)) + 29.0) < 0.5            # 5 % and 3 degrees: the image is 29 dB down
    x = np.random.default_rng(3).standard_normal(64) + 0j
    assert np.array_equal(iq.impair(x, model.GAIN, model.PHASE), model.impair(x))
    sums = [np.array([0.1, -0.05, 3.0]), np.array([0.4, 0.02, 9.0])]
    assert iq.beta_from_sums(sums[0]) == model.finish(sums[0])
    assert iq.balance_from(sums) == model.finish(sums[0] + sums[1])
    assert iq.balance_from([(0j, s) for s in sums]) == model.finish(sums[0] + sums[1])      # what Tuner.iq_imbalance returns
    with pytest.raises(ValueError):
        iq.balance_from([])
    assert iq.pair_range(90001) == (1, 45000) and iq.pair_range(600000) == (1, 299999) and iq.pair_range(3) == (1, 1)
    assert iq.pair_range(90001, 100.4, 2000.0) == (100, 1999)
    for bad in (dict(n=2), dict(n=1), dict(n=100, f_lo=0), dict(n=100, f_hi=51), dict(n=100, f_lo=20, f_hi=20),
                dict(n=100, f_lo=-3, f_hi=5)):
        with pytest.raises(ValueError):
            iq.pair_range(**bad)


@pytest.mark.parametrize("n", [3, 4, 5, 8, 9])
def test_index_rules(n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    k = np.arange(n)
    assert np.array_equal(model.mirror(n), (-k) % n) and model.mirror(n)[0] == 0
    self_mirrored = [int(i) for i in k if model.mirror(n)[i] == i]
    assert self_mirrored == ([0, n // 2] if n % 2 == 0 else [0])
    assert model.last_pair(n) == (n - 1) // 2 and all(m != n - m for m in range(1, model.last_pair(n) + 1))
    # the pairs never touch the self-mirrored bins: whatever sits there does not move the sums
    sums, _ = model.estimate_sums(X)
    Z = X.copy()
    Z[self_mirrored] += 1e6
    assert np.array_equal(model.estimate_sums(Z)[0], sums)
    by_hand = sum(X[m] * X[n - m] for m in range(1, model.last_pair(n) + 1))
    assert np.isclose(sums[0] + 1j * sums[1], by_hand)
    for bad in ((0, 1), (1, model.last_pair(n) + 1), (2, 1)):
        with pytest.raises(ValueError):
            model.estimate_sums(X, *bad)
    # the correction: self-mirrored bins use themselves; the notch of half-width w takes signed bins |s| <= w - 1
    beta = 0.03 - 0.02j
    Y = model.correct(X, beta)
    for i in range(n):
        assert np.isclose(Y[i], X[i] - beta * np.conj(X[(n - i) % n]))
    assert model.notch_bins(n, 0).size == 0 and list(model.notch_bins(n, 1)) == [0]
    if n >= 4:
        assert list(model.notch_bins(n, 2)) == [0, 1, n - 1]
    w = n // 2
    Yn = model.correct(X, beta, w)
    zeroed = sorted({s % n for s in range(-(w - 1), w)})
    assert all(Yn[i] == 0 for i in zeroed) and all(Yn[i] == Y[i] for i in range(n) if i not in zeroed)
    if n % 2 == 0:
        assert n // 2 not in zeroed               # the widest notch leaves bin n / 2
    H = model.with_halos(Y, 1)
    assert H[0] == Y[n - 1] and H[-1] == Y[0] and np.array_equal(H[1:-1], Y)


def test_band_restriction_is_the_full_estimate_restricted_by_hand():
    n = 4001
    X = np.fft.fft(model.received(n, seed=5))
    lo, hi = 300, 1200
    sums, cross = model.estimate_sums(X, lo, hi)
    Z = np.zeros_like(X)
    keep = np.arange(lo, hi + 1)
    Z[keep], Z[n - keep] = X[keep], X[n - keep]
    full, cross_full = model.estimate_sums(Z)
    assert np.allclose(sums, full, rtol=1e-13, atol=0) and np.isclose(cross, cross_full, rtol=1e-13)


def _quality(x):
    """|beta_hat - beta| / |beta| of the model's full-band estimate on the buffer x."""
    _, beta = model.balance(np.fft.fft(x))
    true = model.receiver()[2]
    return abs(beta - true) / abs(true)


@pytest.mark.parametrize("name", sorted(model.FIXTURES))
def test_estimator_quality_on_the_gpu_test_inputs(name):
    """A condition on the fixtures, not a measurement: the blind estimate lands within 2 % of the true beta on every input
    the GPU tests load -- as complex64, and for the end-to-end band also as cu8 and cs16."""
    x = model.fixture(name)
    q = [("complex64", _quality(x.astype(np.complex64).astype(np.complex128)))]
    if name == "fast":
        q.append(("cu8", _quality(model.from_cu8(model.quantise_cu8(x)))))
        q.append(("cs16", _quality(model.from_cs16(model.quantise_cs16(x)))))
    print(name, ", ".join("%s %.3g" % kv for kv in q))
    for what, v in q:
        assert v <= model.QUALITY, (name, what, v)


def test_mirrored_carriers_corrupt_the_blind_estimate_and_a_band_without_them_does_not():
    """The documented limit: two unmodulated carriers at exactly mirrored frequencies correlate like an image does."""
    n = 90001
    k = 7000                                         # outside every station and every station's mirror
    x = model.received(n, seed=11, carriers=[(+k, 70.0), (-k, 70.0)])
    X = np.fft.fft(x.astype(np.complex64).astype(np.complex128))
    true = model.receiver()[2]
    full = model.finish(model.estimate_sums(X)[0])
    assert abs(full - true) > model.QUALITY * abs(true), abs(full - true) / abs(true)
    banded = model.finish(model.estimate_sums(X, 8000, model.last_pair(n))[0])
    assert abs(banded - true) <= model.QUALITY * abs(true), abs(banded - true) / abs(true)
