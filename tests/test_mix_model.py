"""CPU: the audio buses' model (tests/mix_model.py) against its own restatement; the three wrong models -- another order,
another rounding -- differ from it on every input the GPU test compares exactly, so a kernel that took one of those
shortcuts cannot pass there; none of those inputs produces a denormal; ``Bus.of``'s gains; every refusal of ``Bus`` and
``Mixer``.  None of this needs a device.

The inputs meant are the seeded ones of mix_model.cases(), which tests/test_hip_mix.py runs the kernel on.  Its Tuner tests
mix audio that only the device has; their buses hold at most 16 channels, where the segmented and the unsegmented order
coincide, and they check the plumbing, not the order."""

import numpy as np
import pytest

import mix_model as mm


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("ch_in,ch_out", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_model_equals_restatement(ch_in, ch_out):
    """Small inputs of every leg combination: route counts around the segment length, a mask, a sub-range, a closed bus."""
    for k, (A, first, masked) in enumerate([(1, 0, True), (5, 3, True), (7, 0, False)]):
        c = mm.Case("small", 100 + 10 * k + 2 * ch_in + ch_out, (0, 1, 15, 16, 17, 33, 40, 5), 48, A, ch_in, ch_out, first=first,
                    masked=masked, closed_bus=7 if masked else None, nan_closed=masked)
        out, active, bus_open = c.want()
        assert out.dtype == np.float32 and out.shape == (8, A, ch_out)
        assert np.array_equal(_bits(out), _bits(mm.mix_restated(*c.args())))
        assert np.isfinite(out).all()                                   # the NaNs of the closed rows reached nothing
        opened = np.ones(48, bool) if c.open is None else c.open != 0
        want_active = [int(opened[c.chan[c.bus_start[m]:c.bus_start[m + 1]] - first].sum()) for m in range(8)]
        assert active.tolist() == want_active and bus_open.tolist() == [int(n > 0) for n in want_active]
        assert active[0] == 0 and not _bits(out[0]).any()               # a bus without a route: +0
        if masked:
            assert active[7] == 0 and not _bits(out[7]).any()           # a bus whose routes are all closed: +0


def test_the_sum_of_negative_zeros_is_positive_zero():
    """Every sum starts from +0: a bus of -0 samples gives +0, as the device's add does."""
    audio = np.full((3, 4, 1), -0.0, np.float32)
    out, _, _ = mm.mix(audio, None, 0, [0, 3], [0, 1, 2], np.ones((3, 2), np.float32), 2)
    assert not _bits(out).any()


@pytest.mark.parametrize("case", mm.cases(), ids=lambda c: c.name)
def test_wrong_models_differ_and_nothing_is_denormal(case):
    """Each of the three wrong models differs from the model in at least 10 % of the output samples; no product and no
    partial sum is a nonzero float32 denormal, so the result does not depend on the denormal mode."""
    tiny = np.finfo(np.float32).tiny
    worst = [np.inf]

    def watch(a):
        nz = np.abs(a[(a != 0) & np.isfinite(a)])
        if nz.size:
            worst[0] = min(worst[0], float(nz.min()))
    out, _, _ = mm.mix(*case.args(), watch=watch)
    assert np.array_equal(_bits(out), _bits(case.want()[0]))
    assert worst[0] >= tiny, worst[0]
    assert np.isfinite(out).all()
    for name, wrong in mm.WRONG.items():
        share = float(np.mean(_bits(wrong(*case.args())) != _bits(out)))
        print("%s, %s: differs in %.1f %% of the samples" % (case.name, name, 100.0 * share))
        assert share >= 0.10, (case.name, name, share)


def test_bus_of_gains_match_float64():
    import radiocore as rc
    from radiocore.tools import mix as rmix
    rng = np.random.default_rng(5)
    chans = rng.choice(500, size=40, replace=False)
    db, pan = rng.uniform(-12.0, 6.0, 40), rng.uniform(-1.0, 1.0, 40)
    bus = rc.Bus.of(chans, gain_db=db, pan=pan, name="tower")
    gl, gr = mm.pan_gains(db, pan)
    assert bus.gains.dtype == np.float32 and bus.channels.dtype == np.int32 and bus.channels.tolist() == chans.tolist()
    assert np.array_equal(bus.gains[:, 0], gl.astype(np.float32)) and np.array_equal(bus.gains[:, 1], gr.astype(np.float32))
    assert bus.name == "tower" and len(bus) == 40
    # constant power: gl^2 + gr^2 = g^2; centre: both sides 3 dB down; hard left and right
    assert np.allclose(gl ** 2 + gr ** 2, 10.0 ** (db / 10.0), rtol=1e-12)
    c = rc.Bus.of([4], gain_db=0.0, pan=0.0)
    assert np.allclose(c.gains, np.sqrt(0.5), rtol=1e-7)
    assert np.allclose(rc.Bus.of([4], pan=-1.0).gains, [[1.0, 0.0]], atol=1e-7)
    assert np.allclose(rc.Bus.of([4], pan=1.0).gains, [[0.0, 1.0]], atol=1e-7)
    # balance: the stereo form, one side untouched
    bal = rng.uniform(-1.0, 1.0, 40)
    b2 = rc.Bus.of(chans, gain_db=db, balance=bal)
    gl, gr = mm.balance_gains(db, bal)
    assert np.array_equal(b2.gains[:, 0], gl.astype(np.float32)) and np.array_equal(b2.gains[:, 1], gr.astype(np.float32))
    assert rc.Bus.of([1, 2], gain_db=-6.0, balance=0.0).gains.tolist() == [[np.float32(10.0 ** -0.3)] * 2] * 2
    assert rc.Bus.of([1], balance=-1.0).gains.tolist() == [[1.0, 0.0]] and rc.Bus.of([1], balance=0.5).gains.tolist() == [[0.5, 1.0]]
    # scalars for all, an empty bus, the module's helpers
    assert rc.Bus.of([3, 9], gain_db=6.0, pan=0.25).gains[0].tolist() == rc.Bus.of([3], gain_db=6.0, pan=0.25).gains[0].tolist()
    assert len(rc.Bus.of([])) == 0 and len(rc.Bus([])) == 0
    assert np.allclose(np.stack(rmix.pan_gains(2.0, pan)), np.stack(mm.pan_gains(20.0 * np.log10(2.0), pan)), rtol=1e-14, atol=0.0)
    assert np.allclose(np.stack(rmix.balance_gains(2.0, bal)), np.stack(mm.balance_gains(20.0 * np.log10(2.0), bal)), rtol=1e-14, atol=0.0)


def test_bus_and_mixer_refusals():
    import radiocore as rc
    from radiocore.tools.mix import Bus, Mixer
    assert rc.Bus is Bus and rc.Mixer is Mixer
    ok = Bus([(0, 1.0, 0.5), (3, 0.25, 0.0)])
    assert ok.channels.tolist() == [0, 3] and ok.gains.tolist() == [[1.0, 0.5], [0.25, 0.0]]
    for bad in ([(0, 1.0)], [(0, 1.0, 1.0, 1.0)], [5], [("a", 1.0, 1.0)], [(0, "x", 1.0)], [(0.5, 1.0, 1.0)],
                [(-1, 1.0, 1.0)], [(2 ** 31, 1.0, 1.0)],
                [(0, float("nan"), 1.0)], [(0, 1.0, float("inf"))], [(0, 1e39, 1.0)],        # (1e39 is inf as float32)
                [(0, 1.0, 1.0), (1, 1.0, 1.0), (0, 0.5, 0.5)],                               # a channel twice
                [(c, 1.0, 1.0) for c in range(65536)]):
        with pytest.raises(ValueError):
            Bus(bad)
    assert len(Bus([(c, 1.0, 1.0) for c in range(65535)])) == 65535
    for bad in (dict(pan=1.5), dict(pan=-1.01), dict(balance=2.0), dict(pan=0.5, balance=0.5), dict(gain_db=float("nan")),
                dict(gain_db=float("inf")), dict(pan=float("nan")), dict(gain_db=[0.0, 1.0]), dict(pan=[0.0] * 4),
                dict(balance=[[0.0] * 3])):
        with pytest.raises(ValueError):
            Bus.of([1, 2, 3], **bad)
    with pytest.raises(ValueError):
        Bus.of([1, 1])
    with pytest.raises(ValueError):
        Bus.of([1], gain_db=2000.0)                                      # the gain overflows float32
    # Mixer: 1 .. 1024 buses of Bus, at most 2^20 routes
    for bad in ([], [ok] * 1025, [ok, "bus"], [[(0, 1.0, 1.0)]]):
        with pytest.raises(ValueError):
            Mixer(bad)
    big = Bus([(c, 1.0, 1.0) for c in range(65535)])
    with pytest.raises(ValueError):
        Mixer([big] * 17)                                                # 17 x 65 535 > 2^20
    m = Mixer([big] * 16 + [Bus([(c, 1.0, 1.0) for c in range(16)])])    # exactly 2^20
    assert m.M == 17 and m.ch_out == 2 and m.highest_channel() == 65534
    assert Mixer([ok], stereo=False).ch_out == 1 and Mixer([Bus([])]).highest_channel() == -1
    # the tables per launch group: a bus belongs to one group; a channel the tuner does not have is refused
    a, b, e = Bus.of([0, 2], name="low"), Bus.of([5, 4]), Bus([])
    owner, tables = Mixer([a, b, e])._split(((0, 3), (3, 3)), 6)
    assert owner == [0, 1, 0]
    assert tables[0][0].tolist() == [0, 2, 2, 2] and tables[0][1].tolist() == [0, 2]
    assert tables[1][0].tolist() == [0, 0, 2, 2] and tables[1][1].tolist() == [5, 4] and tables[1][2].shape == (2, 2)
    with pytest.raises(ValueError, match="low"):
        Mixer([a])._split(((0, 2),), 2)                                  # channel 2 of a tuner with two
    with pytest.raises(ValueError, match="launch groups"):
        Mixer([Bus.of([2, 3])])._split(((0, 3), (3, 3)), 6)
