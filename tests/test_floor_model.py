"""The noise floor's model (tests/floor_model.py) pinned against its own restatement, the properties the GPU tests' tolerances
rest on, the host-side pieces of the feature (NoiseFloor's conversions, the channel gain G, spectrum.occupied with a floor),
and the margins of the Tuner scene.  No device."""

import numpy as np
import pytest

import floor_model as fm
import squelch_model


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _awkward(rng, M):
    """float32 [M]: four levels (heavy in ties) with +-0, denormals, +-inf and NaNs of both signs sprinkled in."""
    x = rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=M)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan, -np.nan, -3.0], np.float32)
    hit = rng.random(M) < 0.3
    x[hit] = rng.choice(special, size=int(hit.sum()))
    return x


def test_ordering_rule():
    x = np.array([np.nan, np.inf, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -np.inf], np.float32)
    k = fm.keys(x)
    assert np.all(np.diff(k[1:].astype(np.int64)) < 0)                  # descending as listed: -0 below +0, -inf lowest
    assert k[0] > k[1]                                                  # NaN above +inf
    neg_nan = np.array([0xffc00001], np.uint32).view(np.float32)
    assert fm.keys(neg_nan)[0] == k[0] == 0xffffffff                    # every NaN the same key, whatever its sign and payload
    back = fm.values(k)
    assert np.array_equal(_bits(back)[1:], _bits(x)[1:]) and _bits(back)[0] == 0x7fc00000
    # the rank filter hands out the input's bits: -0 stays -0, and a NaN comes out as 0x7fc00000
    out = fm.rank_filter(np.array([-0.0, 0.0, -0.0, neg_nan[0]], np.float32), 1, 0, 0)
    assert _bits(out).tolist() == [0x00000000, 0x80000000, 0x00000000, 0x80000000]
    out = fm.rank_filter(np.array([-0.0, 0.0, -0.0, neg_nan[0]], np.float32), 1, 0, 1000)
    assert _bits(out).tolist() == [0x00000000, 0x80000000, 0x7fc00000, 0x80000000]


@pytest.mark.parametrize("M,half,guard", [(2, 1, 0), (3, 1, 0), (3, 2, 1), (4, 2, 1), (9, 7, 6), (40, 7, 0), (40, 7, 3), (40, 64, 5),
                                          (130, 63, 62), (67, 65, 1)])
def test_rank_filter_against_restatement(M, half, guard):
    rng = np.random.default_rng(1000 * M + 10 * half + guard)
    for x in (_awkward(rng, M), rng.exponential(1.0, M).astype(np.float32), np.full(M, 3.0, np.float32)):
        for q in (0, 1, 250, 500, 999, 1000):
            got, want = fm.rank_filter(x, half, guard, q), fm.rank_filter_restated(x, half, guard, q)
            assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), (M, half, guard, q)


def test_rank_rule_at_shortened_windows():
    """cnt and r cell by cell at the band ends; q = 0 / 1000 are the minimum / maximum of exactly the candidates."""
    x = np.arange(10, dtype=np.float32)
    assert fm.counts(10, 3, 1).tolist() == [2, 2, 3, 4, 4, 4, 4, 3, 2, 2]
    assert fm.rank_filter(x, 3, 1, 0).tolist() == [2, 3, 0, 0, 1, 2, 3, 4, 5, 6]
    assert fm.rank_filter(x, 3, 1, 1000).tolist() == [3, 4, 5, 6, 7, 8, 9, 9, 6, 7]
    # r = (q (cnt - 1)) / 1000, integer division: q = 999 is below the maximum unless cnt = 1; q = 500 the lower median
    assert fm.ranks([1, 2, 3, 4, 96], 999).tolist() == [0, 0, 1, 2, 94]
    assert fm.ranks([1, 2, 3, 4, 96], 500).tolist() == [0, 0, 1, 1, 47]
    assert fm.rank_filter(x, 3, 1, 500).tolist() == [2, 3, 4, 1, 2, 3, 4, 5, 5, 6]
    # M = guard + 2 is accepted; the cells between the ends have no candidate and get NaN
    assert fm.counts(3, 2, 1).tolist() == [1, 0, 1]
    out = fm.rank_filter(np.array([5.0, 6.0, 7.0], np.float32), 2, 1, 500)
    assert _bits(out).tolist() == [_bits(np.float32(7.0))[()], 0x7fc00000, _bits(np.float32(5.0))[()]]
    # a window of NaN only gives NaN; one number among NaNs is every rank below the top
    x = np.full(9, np.nan, np.float32)
    assert np.all(_bits(fm.rank_filter(x, 2, 0, 500)) == 0x7fc00000)
    x[4] = 2.0
    assert fm.rank_filter(x, 2, 0, 0)[2:7].tolist()[0:2] == [2.0, 2.0] and np.isnan(fm.rank_filter(x, 2, 0, 0)[4])


def test_rank_filter_is_monotone_and_scale_equivariant():
    """What carries a relative error bound of the power spectrum through the filter: x <= y cell by cell gives
    filter(x) <= filter(y), and filter(c x) = c filter(x) for c > 0 -- so y within [x (1 - eps), x (1 + eps)] gives
    filter(y) within [filter(x) (1 - eps), filter(x) (1 + eps)]."""
    rng = np.random.default_rng(7)
    x = rng.exponential(1.0, 500)
    eps = 6e-6
    y = x * (1.0 + eps * rng.uniform(-1.0, 1.0, 500))
    for half, guard, q in ((7, 0, 250), (60, 12, 250), (64, 4, 500), (300, 1, 999)):
        fx, fy = fm.rank_filter64(x, half, guard, q), fm.rank_filter64(y, half, guard, q)
        assert np.all(fm.rank_filter64(x * (1.0 + eps), half, guard, q) >= fy) and np.all(fm.rank_filter64(x * (1.0 - eps), half, guard, q) <= fy)
        assert np.array_equal(fm.rank_filter64(4.0 * x, half, guard, q), 4.0 * fx)           # (a power of two: exact)
        assert np.max(np.abs(fy / fx - 1.0)) <= eps * (1.0 + 1e-12)
    # float32 and float64 agree on float32 data: the order statistic picks an input value
    x32 = x.astype(np.float32)
    assert np.array_equal(fm.rank_filter(x32, 60, 12, 250).astype(np.float64), fm.rank_filter64(x32, 60, 12, 250))


def test_three_runs_with_state():
    rng = np.random.default_rng(11)
    M, half, guard, q = 300, 20, 3, 250
    rise, fall = np.float32(fm.factor(10.0)), np.float32(fm.factor(1.0))
    s = np.full(M, np.nan, np.float32)
    p1 = rng.exponential(1.0, M).astype(np.float32)
    s1, over1 = fm.floor_run(s, p1, half, guard, q, rise, fall, 4.0)
    e1 = fm.rank_filter(p1, half, guard, q)
    assert np.array_equal(_bits(s1), _bits(e1))                                    # not primed: the estimate as it is
    p2 = (4.0 * p1).astype(np.float32)                                             # the floor rises: the slow factor
    s2, _ = fm.floor_run(s1, p2, half, guard, q, rise, fall, 4.0)
    want = (s1 + (rise * ((4.0 * e1).astype(np.float32) - s1)).astype(np.float32)).astype(np.float32)
    assert np.array_equal(_bits(s2), _bits(want)) and np.all(s2 > s1) and np.all(s2 < 4.0 * e1)
    p3 = (0.25 * p1).astype(np.float32)                                            # ... and falls: the fast one
    s3, over3 = fm.floor_run(s2, p3, half, guard, q, rise, fall, 4.0)
    want = (s2 + (fall * ((0.25 * e1).astype(np.float32) - s2)).astype(np.float32)).astype(np.float32)
    assert np.array_equal(_bits(s3), _bits(want)) and np.all(s3 < s2)
    assert np.array_equal(over3, (p3 >= (np.float32(4.0) * s3).astype(np.float32)).astype(np.uint8))
    assert 0 < int(over1.sum()) < M // 2                        # exponential cells: a third lie 6 dB over their lower quartile
    # a NaN estimate leaves the state as it was, a NaN state takes the estimate; over is false on NaN
    pn = np.full(M, np.nan, np.float32)
    s4, over4 = fm.floor_run(s3, pn, half, guard, q, rise, fall, 4.0)
    assert np.array_equal(_bits(s4), _bits(s3)) and not over4.any()
    # equality: a cell whose power equals ratio s' is over
    s5, over5 = fm.floor_run(np.full(M, np.nan, np.float32), np.full(M, 2.0, np.float32), half, guard, q, rise, fall, 1.0)
    assert np.all(s5 == 2.0) and over5.all()
    # rise = fall = 1: no memory
    s6, _ = fm.floor_run(s3, p1, half, guard, q, 1.0, 1.0, 4.0)
    assert np.allclose(s6, e1, rtol=2e-7)


def test_thresholds():
    floor = np.array([1.0, 2.0, np.nan, 3.0], np.float32)
    cell = np.array([0, 3, 3, 2, -1, 4, 1], np.int32)
    gain = np.array([0.1, 0.1, 7.0, 1.0, 1.0, 1.0, np.float32(1.0 / 3.0)], np.float32)
    thr = fm.thresholds(floor, cell, gain)
    assert thr.dtype == np.float32
    want = [np.float32(1.0) * np.float32(0.1), np.float32(3.0) * np.float32(0.1), np.float32(21.0)]
    assert thr[:3].tolist() == [float(w) for w in want]
    assert np.isnan(thr[3:6]).all() and thr[6] == np.float32(2.0) * np.float32(1.0 / 3.0)
    # a NaN threshold keeps squelch and gate closed
    assert not squelch_model.open_mask([1e30, 1e30, 1e30], thr[3:6]).any()


def test_channel_gain_against_the_level_definition():
    """G(B, n) = the expected level of a channel over white noise of unit power per bin.  The level is sum w_k^2 E_k with
    E_k = |X_k|^2 / n^2 exponential (mean 1, variance 1): mean G, variance sum w_k^4.  Over R independent draws the mean level
    lies within 5 standard errors, 5 sqrt(sum w^4 / R) / G, of G -- below 5 % for the cases below -- except once in
    1.7 million cases."""
    import radiocore_oracle as oracle
    from radiocore.tools.floor import channel_noise_gain
    rng = np.random.default_rng(5)
    R = 40
    for n, B, roll in ((8000, 2000, 0), (8000, 2000, 3100), (8000, 1001, -777), (6001, 500, 40), (4000, 4000, 0)):
        G = fm.channel_gain(B, n)
        assert abs(channel_noise_gain(B, n) / G - 1.0) < 1e-12
        k = np.concatenate([np.arange(0, B // 2 + 1), n - np.arange(1, B - B // 2), [n - B // 2] if B % 2 == 0 and 2 < B < n else []])
        w2 = (0.5 - 0.5 * np.cos(2.0 * np.pi * ((k - n // 2) % n) / n)) ** 2
        assert abs(w2.sum() / G - 1.0) < 1e-12
        tol = 5.0 * np.sqrt(np.sum(w2 ** 2) / R) / G
        got = np.mean([squelch_model.level(oracle, (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * n / np.sqrt(2.0),
                                           n, roll, B) for _ in range(R)])
        print("n %d B %d: G %.3f, mean level %.3f, tolerance %.2f %%" % (n, B, G, got, 100.0 * tol))
        assert 0.005 < tol < 0.05 and abs(got / G - 1.0) <= tol


def test_noise_floor_conversions():
    from radiocore.tools.floor import NoiseFloor, OverFloor
    nf = NoiseFloor(100.0)
    assert (nf.half, nf.guard, nf.q) == (64, 4, 250)
    a, b = nf.factors
    assert a.dtype == np.float32 and a == np.float32(1.0 - np.exp(-0.1)) and b == np.float32(1.0 - np.exp(-1.0))
    assert NoiseFloor(100, rise=0, fall=0).factors == (1.0, 1.0)
    assert nf.cells(40000) == 400 and nf.cells(40049) == 400 and nf.cells(40051) == 401 and nf.cells(30) == 1
    assert NoiseFloor(12.5, quantile=0.4996).q == 500 and NoiseFloor(12.5, quantile=1).q == 1000 and NoiseFloor(1, quantile=0).q == 0
    assert NoiseFloor(100, half=4096, guard=4095).guard == 4095
    for bad in (dict(cell_hz=0.5), dict(cell_hz=float("nan")), dict(cell_hz=100, half=0), dict(cell_hz=100, half=4097),
                dict(cell_hz=100, half=2.5), dict(cell_hz=100, guard=-1), dict(cell_hz=100, half=8, guard=8),
                dict(cell_hz=100, quantile=-0.1), dict(cell_hz=100, quantile=1.01), dict(cell_hz=100, quantile=float("nan")),
                dict(cell_hz=100, rise=-1.0), dict(cell_hz=100, fall=float("inf")), dict(cell_hz=100, fall=float("nan"))):
        with pytest.raises(ValueError):
            NoiseFloor(**bad)
    assert OverFloor(10).db == 10.0 and repr(OverFloor(7.5)) == "OverFloor(7.5)"
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            OverFloor(bad)


def test_occupied_with_a_floor():
    from radiocore.tools import spectrum
    rng = np.random.default_rng(3)
    M = 640
    floor = 10.0 ** (2.0 * np.arange(M) / M)                           # a 20 dB tilt
    power = floor * rng.uniform(0.8, 1.25, M)
    power[100:104] *= 10.0 ** 1.2
    power[500:503] *= 10.0 ** 1.2
    power[610] *= 10.0 ** 1.2
    want = [(100, 103), (500, 502), (610, 610)]
    runs = spectrum.occupied(power, 8.0, floor=floor)
    assert [r[:2] for r in runs] == want and all(a <= s <= b for a, b, s in runs)
    assert [r[:2] for r in spectrum.occupied(power, 8.0, min_cells=2, floor=floor)] == want[:2]
    # the global median finds no threshold that does the same: at 8 dB the upper end of the band is all "occupied"
    assert [r[:2] for r in spectrum.occupied(power, 8.0)] != want
    # lengths scale power and floor alike; a NaN floor keeps its cell out; None is today's rule, bit for bit
    assert spectrum.occupied(power, 8.0, lengths=7.0, floor=floor) == runs
    holed = floor.copy()
    holed[101] = np.nan
    assert [r[:2] for r in spectrum.occupied(power, 8.0, floor=holed)] == [(100, 100), (102, 103)] + want[1:]
    density = power
    keep = density >= float(np.median(density)) * 10.0 ** 0.8
    assert sum(b - a + 1 for a, b, _ in spectrum.occupied(power, 8.0, floor=None)) == int(keep.sum())
    with pytest.raises(ValueError):
        spectrum.occupied(power, 8.0, floor=floor[:-1])


@pytest.fixture(scope="module")
def scene():
    """The Tuner scene's float64 truth: per buffer the cells' power, the floor's state, the channels' levels and thresholds."""
    import radiocore_oracle as oracle
    t = fm.tuner_setup(oracle.Tuner(), lambda: oracle.FM(fm.B, fm.A))
    assert t.input_frequency == fm.F_IN and int(t.input_bandwidth) == fm.N
    x = fm.buffer(1)
    t.load(x.astype(np.complex128))
    levels = squelch_model.levels(oracle, t)
    p = fm.cell_power64(x).astype(np.float32)
    s, _ = fm.floor_run(np.full(fm.CELLS, np.nan, np.float32), p, fm.HALF, fm.GUARD, 250, 1.0, 1.0, 1.0)
    return levels, fm.thresholds(s, fm.channel_cells(), fm.gains(fm.OVER_DB)), fm.thresholds(s, fm.channel_cells(), fm.gains(0.0))


def test_scene_margins(scene):
    levels, thr, floor_levels = scene
    stations = np.zeros(fm.C, bool)
    stations[list(fm.STATIONS)] = True
    over = 10.0 * np.log10(levels / floor_levels)
    print("dB over the tracked floor:", np.round(over, 2), " margin %.2f dB" % squelch_model.margin_db(levels, thr))
    assert np.array_equal(squelch_model.open_mask(levels, thr), stations)
    assert squelch_model.margin_db(levels, thr) >= fm.MARGIN_DB                   # every level >= 3 dB from its threshold
    assert np.all(over[stations] >= 13.0) and np.all(np.abs(over[~stations]) < 3.0)
    # no single fixed threshold does it: the loudest empty channel exceeds the weakest station
    assert levels[~stations].max() > levels[stations].min()
