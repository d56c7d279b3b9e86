"""The numpy model of the bus dynamics (tests/busdyn_model.py) against a scalar restatement of include/rcfm.h's definition, the
properties the definition promises, the duck's knots, the conversions of radiocore.Limiter / Duck, and three deliberately
wrong models, each of which must differ from the model on every named burst input.  No device."""

import numpy as np
import pytest

import busdyn_model as bm
from busdyn_model import F32, Params, State


def _three_calls(p, xs, opens=None, run=bm.run, **kw):
    st, outs = State(p), []
    for q, x in enumerate(xs):
        out, open_out, st = run(p, st, x, None if opens is None else opens[q], **kw)
        outs.append((out, open_out, st))
    return outs


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == F32 else a,
                                                                        b.view(np.uint32) if b.dtype == F32 else b)


@pytest.mark.parametrize("M,A,ch,L,ducked", [(3, 150, 2, 8, True), (2, 65, 1, 64, True), (3, 5, 2, 8, False), (1, 37, 1, 9, False),
                                            (4, 100, 2, 16, True)])
def test_model_equals_the_scalar_restatement(M, A, ch, L, ducked):
    rng = np.random.default_rng(M * 1000 + A)
    duck = None
    if ducked:
        duck = (np.array([(m + 1) % M if m % 2 == 0 else -1 for m in range(M)], np.int32), rng.uniform(0.1, 0.9, M).astype(F32),
                rng.uniform(0.0, 0.4, M).astype(F32), rng.integers(0, 4, M).astype(np.int32))
    p = Params(M, ch, L, 0.89, 0.2, *(duck or (None,) * 4))
    xs = [np.stack([bm.make_input(rng, bm.KINDS[(m + q) % 4], A, ch, m, M) for m in range(M)]) for q in range(3)]
    xs[1][0, A // 2, 0] = np.nan                        # a NaN never wins a maximum; it comes out as a NaN sample
    opens = [(rng.random(M) < 0.5).astype(np.uint8) for _ in range(3)]
    for got, want in zip(_three_calls(p, xs, opens), _three_calls(p, xs, opens, run=bm.run_restated)):
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[1], want[1])
        assert _same(got[2].tail, want[2].tail) and _same(got[2].h, want[2].h) and np.array_equal(got[2].hang, want[2].hang)


@pytest.mark.parametrize("A,L,ch", [(1, 8, 1), (100, 8, 2), (1000, 64, 2), (4099, 100, 1), (1000, 2048, 2), (10007, 2048, 1)])
def test_output_never_exceeds_the_ceiling(A, L, ch):
    rng = np.random.default_rng(A + L)
    p = Params(2, ch, L, 0.5, 0.3)
    xs = [(3.0 * rng.standard_normal((2, A, ch))).astype(F32) for _ in range(3)]
    xs[2][0, 0, 0] = F32(3e38)
    for out, _, _ in _three_calls(p, xs):
        assert np.all(np.abs(out) <= p.c)


@pytest.mark.parametrize("A,L,ch", [(1, 8, 1), (5, 8, 2), (63, 64, 1), (1000, 64, 2), (4099, 100, 1), (1000, 2048, 2)])
def test_below_the_ceiling_the_row_is_delayed_bit_for_bit(A, L, ch):
    rng = np.random.default_rng(A * 3 + L)
    p = Params(3, ch, L, 0.89, 0.05)
    xs = [np.stack([bm.make_input(rng, "below", A, ch) for _ in range(3)]) for _ in range(3)]
    xs[0][0, 0, 0] = F32(-0.0)
    outs = _three_calls(p, xs)
    whole = np.concatenate([np.zeros((3, L, ch), F32)] + xs, axis=1)
    got = np.concatenate([o[0] for o in outs], axis=1)
    assert np.array_equal(got.view(np.uint32), whole[:, :3 * A].view(np.uint32))
    assert np.all(outs[-1][2].h == 1.0)


@pytest.mark.parametrize("A,L,ch", [(64, 64, 1), (512, 64, 2), (1000, 8, 2), (300, 100, 1)])
def test_one_call_of_2A_equals_two_calls_of_A(A, L, ch):
    rng = np.random.default_rng(A + 7 * L)
    duck = (np.array([1, -1], np.int32), np.array([0.3, 1.0], F32), np.array([0.2, 0.0], F32), np.array([2, 0], np.int32))
    p = Params(2, ch, L, 0.89, 0.1, *duck)
    x = np.stack([bm.make_input(rng, kind, 2 * A, ch, m, 2) for m, kind in enumerate(("steady", "burst"))])
    whole, _, st2 = bm.run(p, State(p), x)
    a, _, st = bm.run(p, State(p), x[:, :A])
    b, _, st = bm.run(p, st, x[:, A:])
    assert np.array_equal(np.concatenate([a, b], axis=1).view(np.uint32), whole.view(np.uint32))
    assert _same(st.tail, st2.tail) and _same(st.h, st2.h) and np.array_equal(st.hang, st2.hang)


def test_rows_shorter_than_the_block():
    """A < L: the tail is the last L samples of tail ++ row, and what comes out is what went in L samples earlier."""
    rng = np.random.default_rng(5)
    p = Params(1, 2, 64, 0.89, 0.1)
    xs = [np.clip(0.1 * rng.standard_normal((1, A, 2)), -0.8, 0.8).astype(F32) for A in (5, 63, 1, 40, 64, 30)]
    st, got = State(p), []
    for x in xs:
        out, _, st = bm.run(p, st, x)
        got.append(out)
        assert st.tail.shape == (1, 64, 2)
    whole = np.concatenate([np.zeros((1, 64, 2), F32)] + xs, axis=1)
    n = sum(x.shape[1] for x in xs)
    assert np.array_equal(np.concatenate(got, axis=1).view(np.uint32), whole[:, :n].view(np.uint32))
    assert np.array_equal(st.tail, whole[:, n:n + 64])


def test_duck_turns_on_holds_and_releases_at_the_expected_knots():
    """Bus 1 is keyed by bus 0, which talks in blocks 4 .. 6 of 20: Qk covers the two latest blocks, so ducking is on at the
    knots 5 .. 8, the hold of 3 keeps it on for the knots 9 .. 11, and from knot 12 on the gain recovers by the release."""
    L, B = 8, 20
    depth, k = F32(0.25), F32(0.5)
    p = Params(2, 1, L, 0.9, k, [-1, 0], [1.0, depth], [0.0, 0.1], [0, 3])
    x = np.zeros((2, B * L, 1), F32)
    x[0, 4 * L:7 * L] = 0.5
    x[1] = 0.01
    out, _, st = bm.run(p, State(p), x)
    g = out[1, L:, 0] / F32(0.01)                        # the gain of bus 1 at the samples whose source is the row
    knot = {b: g[b * L - 1 - L] for b in range(2, B + 1)}    # the last sample of block b - 1 carries h[b] itself (w = 1)
    for b in range(2, 5):
        assert knot[b] == 1.0
    for b in range(5, 12):
        assert abs(knot[b] - depth) < 1e-6, b
    h = depth
    for b in range(12, B + 1):
        h = F32(h + F32(F32(F32(1) - h) * k))
        assert abs(knot[b] - h) < 1e-6, b
    assert st.hang[1] == 0
    # between two knots the gain is the straight line
    ramp = g[4 * L - L:5 * L - L]
    assert np.allclose(ramp, 1.0 + (depth - 1.0) * np.arange(1, L + 1) / L, atol=1e-6)
    # bus 0 itself is untouched: below the ceiling and not keyed
    assert np.array_equal(out[0, L:, 0], x[0, :-L, 0])


def test_key_chain_uses_the_key_buses_input():
    """0 ducks 1 and 1 ducks 2: bus 2 follows the INPUT of bus 1, whether or not bus 1 is being ducked at the time."""
    L = 8
    p = Params(3, 1, L, 0.9, 0.5, [-1, 0, 1], [1.0, 0.01, 0.5], [0.0, 0.1, 0.1], [0, 0, 0])
    x = np.zeros((3, 10 * L, 1), F32)
    x[0, 3 * L:5 * L] = 0.5
    x[1] = 0.2                                            # over bus 2's threshold throughout, also while ducked to 0.002
    x[2] = 0.05
    out, _, _ = bm.run(p, State(p), x)
    assert np.allclose(out[2, 3 * L:, 0], 0.05 * 0.5, atol=1e-7)
    assert np.allclose(out[1, 5 * L - 1:7 * L - 1:L, 0], 0.2 * 0.01, atol=1e-7)
    # the same through the scalar restatement
    assert np.array_equal(bm.run_restated(p, State(p), x)[0].view(np.uint32), out.view(np.uint32))


def test_open_mask():
    p = Params(3, 1, 8, 0.9, 0.5)
    x = np.zeros((3, 20, 1), F32)
    x[1, 15] = 0.25
    _, o, st = bm.run(p, State(p), x, np.array([0, 1, 0], np.uint8))
    assert o.tolist() == [0, 1, 0]
    _, o, st = bm.run(p, st, np.zeros_like(x), np.zeros(3, np.uint8))
    assert o.tolist() == [0, 1, 0]                        # bus 1 went idle: its tail still holds a sample
    _, o, st = bm.run(p, st, np.zeros_like(x), np.zeros(3, np.uint8))
    assert o.tolist() == [0, 0, 0]
    assert bm.run(p, st, x, None)[1].tolist() == [1, 1, 1]


def test_limiter_and_duck_conversions():
    import radiocore as rc
    for rate, kw in ((8000, {}), (48000, {}), (8000, dict(ceiling_db=-3.0, lookahead=0.0125, release=0.1)), (12000, dict(lookahead=1.0)),
                     (8000, dict(lookahead=1e-5))):
        L, c, k = rc.Limiter(**kw).discretise(rate)
        assert (L, c, k) == bm.limiter_params(float(rate), **kw)
        assert c.dtype == F32 and k.dtype == F32 and 8 <= L <= 2048 and 0 < k <= 1
    assert rc.Limiter().discretise(8000)[0] == 64 and rc.Limiter().discretise(48000)[0] == 384
    assert rc.Limiter().discretise(8000)[1] == F32(10.0 ** -0.05)
    assert rc.Limiter().discretise(8000)[2] == F32(1.0 - np.exp(-64 / 2000.0))
    assert rc.Limiter(lookahead=1.0).discretise(12000)[0] == 2048 and rc.Limiter(lookahead=1e-5).discretise(8000)[0] == 8
    for rate, L, kw in ((8000, 64, {}), (48000, 384, dict(depth_db=-6.0, threshold_db=-20.0, hold=0.0)), (8000, 8, dict(hold=1e6))):
        assert rc.Duck(0, **kw).discretise(rate, L) == bm.duck_params(float(rate), L, **kw)
    d, thr, hold = rc.Duck("tower").discretise(8000, 64)
    assert d == F32(10.0 ** -0.6) and thr == F32(0.01) and hold == 62         # round(0.5 x 8000 / 64 = 62.5) to even
    assert rc.Duck(0, hold=1e6).discretise(8000, 8)[2] == 1 << 15
    for bad in (dict(ceiling_db=np.nan), dict(lookahead=0.0), dict(release=-1.0), dict(ceiling_db=np.inf), dict(ceiling_db="x")):
        with pytest.raises(ValueError):
            rc.Limiter(**bad)
    for bad in (dict(key=1.5), dict(key=None), dict(key=0, depth_db=1.0), dict(key=0, hold=-1.0), dict(key=0, threshold_db=np.nan)):
        with pytest.raises(ValueError):
            rc.Duck(**bad)
    with pytest.raises(ValueError):
        rc.Limiter(release=1e30).discretise(8000)          # k rounds to 0


def test_no_denormal_intermediate_on_the_kernel_test_inputs():
    """Every product, sum and difference of the model on the inputs tests/test_hip_busdyn.py compares exactly is zero or a
    normal float32: the comparison does not depend on how a device treats denormals."""
    worst = [np.inf]

    def watch(a):
        a = np.abs(np.asarray(a))
        nz = a[(a != 0) & np.isfinite(a)]
        if nz.size:
            worst[0] = min(worst[0], float(nz.min()))
    for c in bm.cases():
        c.want(watch=watch)
    assert worst[0] >= bm.TINY, worst[0]


@pytest.mark.parametrize("name", sorted(bm.BURSTS))
@pytest.mark.parametrize("wrong", bm.WRONG)
def test_wrong_models_differ_on_the_burst_inputs(name, wrong):
    p, xs = bm.burst_case(name)
    want = np.concatenate([o[0] for o in _three_calls(p, xs)], axis=1)
    got = np.concatenate([o[0] for o in _three_calls(p, xs, variant=wrong)], axis=1)
    differ = float(np.mean(got.view(np.uint32) != want.view(np.uint32)))
    print("%s, %s: %.1f %% of the samples differ" % (name, wrong, 100.0 * differ))
    assert differ >= 0.02, differ
    assert np.all(np.abs(want) <= p.c)
