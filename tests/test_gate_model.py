"""The frame gate's model (tests/gate_model.py) pinned against its own restatement, the host-side pieces of the feature
(squelch.segments, FrameGate's conversions), and the margin the GPU tests' exact mask comparison rests on.  No device."""

import numpy as np
import pytest

import gate_model as gm


def _powers(rng, count, F):
    """float32 [count, F] around thresholds 1.0 / 0.5, with values equal to each threshold and NaNs sprinkled in."""
    p = rng.choice(np.array([0.1, 0.3, 0.5, 0.7, 1.0, 2.0, np.nan], dtype=np.float32), size=(count, F),
                   p=[0.25, 0.2, 0.1, 0.2, 0.1, 0.1, 0.05])
    return p


@pytest.mark.parametrize("hang", [0, 1, 3])
@pytest.mark.parametrize("lead", [0, 1, 2, 7, 50])
def test_state_machine_against_restatement(hang, lead):
    rng = np.random.default_rng(100 * hang + lead)
    for F in (1, 2, 7):
        count = 40
        p = _powers(rng, count, F)
        state = np.stack([rng.integers(0, 2, count), rng.integers(0, hang + 1, count)], axis=1).astype(np.int32)
        to = np.where(rng.random(count) < 0.1, np.nan, 1.0).astype(np.float32)
        got = gm.gate_run(state, p, to, np.float32(0.5), hang, lead)
        want = gm.gate_run_restated(state, p, to, np.float32(0.5), hang, lead)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        assert np.array_equal(got[0][:, 0], (state[:, 0] != 0).astype(np.uint8))


def test_state_machine_cases():
    """Equality opens and holds; NaN neither opens nor holds; hang = 0 closes with the first frame below close; the stored
    state is the undilated one; lead >= F opens the whole buffer before any open frame."""
    one = np.zeros((1, 2), np.int32)
    m, a, s = gm.gate_run(one, [[0.5, 1.0, 0.5, 0.4, 0.4]], 1.0, 0.5, 0, 0)
    assert m.tolist() == [[0, 0, 1, 1, 0, 0]] and a.tolist() == [1] and s.tolist() == [[0, 0]]
    m, a, s = gm.gate_run(one, [[2.0, np.nan, np.nan, np.nan]], 1.0, 0.5, 1, 0)
    assert m.tolist() == [[0, 1, 1, 0, 0]] and s.tolist() == [[0, 0]]
    m, a, s = gm.gate_run(one, [[0.1, 0.1, 0.1, 2.0]], np.nan, 0.5, 1, 0)
    assert m.tolist() == [[0, 0, 0, 0, 0]] and a.tolist() == [0]
    m, a, s = gm.gate_run(one, [[0.1, 0.1, 0.1, 2.0]], 1.0, 0.5, 2, 9)
    assert m.tolist() == [[0, 1, 1, 1, 1]] and s.tolist() == [[1, 2]]
    m, a, s = gm.gate_run(one, [[0.1, 0.1, 2.0, 0.1]], 1.0, 0.5, 0, 1)
    assert m.tolist() == [[0, 0, 1, 1, 0]] and s.tolist() == [[0, 0]]
    # a channel that closed exactly at the buffer edge: column 0 alone keeps open_any up
    m, a, s = gm.gate_run(np.array([[1, 0]], np.int32), [[0.1, 0.1]], 1.0, 0.5, 0, 0)
    assert m.tolist() == [[1, 0, 0]] and a.tolist() == [1] and s.tolist() == [[0, 0]]


@pytest.mark.parametrize("hang", [0, 2])
def test_two_buffers_equal_one_of_twice_the_frames(hang):
    rng = np.random.default_rng(hang)
    F, count = 6, 64
    p = _powers(rng, count, 2 * F)
    zero = np.zeros((count, 2), np.int32)
    whole, _, end = gm.gate_run(zero, p, 1.0, 0.5, hang, 0)
    m0, _, s0 = gm.gate_run(zero, p[:, :F], 1.0, 0.5, hang, 0)
    m1, _, s1 = gm.gate_run(s0, p[:, F:], 1.0, 0.5, hang, 0)
    assert np.array_equal(np.concatenate([m0, m1[:, 1:]], axis=1), whole)
    assert np.array_equal(m1[:, 0], m0[:, -1]) and np.array_equal(s1, end)


@pytest.mark.parametrize("A,F,ch,R", [(40, 5, 1, 0), (40, 5, 1, 3), (40, 5, 2, 8), (35, 7, 1, 5), (12, 1, 2, 12)])
def test_apply_against_restatement(A, F, ch, R):
    rng = np.random.default_rng(A + R)
    count = 32
    x = rng.standard_normal((count, A) + ((ch,) if ch == 2 else ())).astype(np.float32)
    mask = rng.integers(0, 2, (count, F + 1)).astype(np.uint8)
    x[0, 3] = x[1, A - 1] = np.nan
    r = gm.ramp(R)
    got, want = gm.gate_apply(x, mask, r), gm.gate_apply_restated(x, mask, r)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    La = A // F
    for c in range(count):
        for f in range(F):
            seg, src = got[c, f * La:(f + 1) * La], x[c, f * La:(f + 1) * La]
            if mask[c, f + 1] and mask[c, f]:
                assert np.array_equal(seg.view(np.uint32), src.view(np.uint32))
            if not mask[c, f + 1] and not mask[c, f]:
                assert not seg.view(np.uint32).any()                    # +0.0, whatever was there


def test_ramp():
    r = gm.ramp(16)
    assert r.dtype == np.float32 and np.all(np.diff(r) > 0) and 0.0 < r[0] and r[-1] < 1.0
    assert np.allclose(r + r[::-1], 1.0, atol=1e-7)
    assert gm.ramp(0).shape == (0,)


def test_frame_power_model():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 23)) + 1j * rng.standard_normal((3, 23))).astype(np.complex64)
    p = gm.frame_power(x, 5)
    assert p.shape == (3, 4) and p.dtype == np.float64
    want = [[sum(abs(complex(v)) ** 2 for v in x[r, 5 * f:5 * f + 5]) / 5 for f in range(4)] for r in range(3)]
    assert np.allclose(p, want, rtol=1e-12)
    assert np.allclose(gm.frame_power(x.real.copy(), 23)[:, 0], np.mean(x.real.astype(np.float64) ** 2, axis=1), rtol=1e-12)


def test_segments():
    from radiocore.tools import squelch
    m = np.array([[0, 1, 1, 0, 1], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 1]], bool)
    assert squelch.segments(m, 800) == [(0, 160, 480), (0, 640, 800), (1, 0, 800), (3, 0, 160), (3, 640, 800)]
    assert squelch.segments(np.zeros((0, 5), bool), 800) == []
    for bad in (dict(frame_mask=m, A=801), dict(frame_mask=m[0], A=800), dict(frame_mask=m, A=0)):
        with pytest.raises(ValueError):
            squelch.segments(**bad)


def test_frame_gate_conversions():
    import radiocore as rc
    from radiocore.tools.gate import FrameGate
    assert rc.FrameGate is FrameGate
    g = FrameGate()
    assert (g.frames, g.hang_frames, g.lead) == (50, 12, 1)              # round(0.25 * 50) = round(12.5): to even
    assert g.ramp_samples(8000) == 40 and g.ramp_samples(48000) == 240
    assert FrameGate(frames=gm.FRAMES, hang=gm.HANG, ramp=gm.RAMP).hang_frames == 3
    assert FrameGate(frames=10, ramp=0.5).ramp_samples(800) == 80        # capped at one frame
    assert FrameGate(frames=10, ramp=0.0).ramp_array(800).shape == (0,)
    assert np.array_equal(FrameGate(frames=10, ramp=0.02).ramp_array(800), gm.ramp(16))
    with pytest.raises(ValueError):
        g.ramp_samples(8001)
    with pytest.raises(ValueError):
        g.fits(12501)
    for bad in (dict(frames=0), dict(frames=2.5), dict(frames=65536), dict(hang=-1.0), dict(hang=float("nan")),
                dict(lead=-1), dict(lead=0.5), dict(ramp=-0.001), dict(ramp=float("inf"))):
        with pytest.raises(ValueError):
            FrameGate(**bad)


def _oracle_tuner(scene):
    import radiocore_oracle as oracle
    return scene.add_to(oracle.Tuner())


@pytest.mark.parametrize("name", ["FM", "AM", "mixed", "stereo"])
def test_margin_of_the_tuner_buffers(name):
    """What tests/test_hip_gate.py compares exactly: the model's masks of the keyed stations.  Every model frame power lies
    at least 3 dB from both of its thresholds, so no rounding of the device's levels can flip a frame; and the masks show
    what the buffers were built to show."""
    scene = {"mixed": gm.mixed, "stereo": gm.stereo}.get(name, lambda: gm.narrow(name))()
    ref = _oracle_tuner(scene)
    powers, worst = scene.powers(ref, scene.buffers(ref.input_frequency))
    print("%s: the closest frame power lies %.2f dB from a threshold" % (name, worst))
    assert worst >= gm.MARGIN_DB
    masks, anys = scene.masks(powers)
    got = np.concatenate([m[:, 1:] for m in masks], axis=1).astype(bool)
    hang = int(round(gm.HANG * gm.FRAMES))
    want = np.zeros_like(got)
    for c, runs in enumerate(scene.keyed):
        for lo, hi in runs:
            first = lo - gm.LEAD if lo % gm.FRAMES >= gm.LEAD else lo - lo % gm.FRAMES       # look-ahead stops at the buffer's start
            want[c, first:hi + 1 + hang] = True
    assert np.array_equal(got, want)
    assert [a.tolist() for a in anys] == [(m != 0).any(axis=1).astype(int).tolist() for m in masks]
    if name in ("FM", "AM"):
        assert masks[1][4, 0] == 1 and masks[2][7, 0] == 0
        # a station that joins with the second buffer starts closed
        late, _ = scene.masks(powers[1:], stations=[3, 4])
        assert late[0][:, 0].tolist() == [0, 0] and late[0][0, 1:4].tolist() == [1, 1, 1] and not late[0][1].any()
