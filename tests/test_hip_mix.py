"""GPU: the audio buses (include/rcfm.h, "audio buses") against tests/mix_model.py.

rcfm_mix_run: output bits equal the model's -- every product and sum is one float32 rounding in a stated order, so there is
no tolerance.  tests/test_mix_model.py shows, on these very inputs, that a kernel with another order (no segments, segments
of 32) or another rounding (an fma) differs from the model in a quarter of the samples or more.
Through the Tuner: mix() equals the model applied to the same run's audio and open_mask(), bit for bit, behind every kind of
squelch the Tuner has; payloads drained with buses=True equal the model's quantisation.
"""

import ctypes

import numpy as np
import pytest

import mix_model as mm
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ERR_ARG, ERR_INDEX = -4, -2
_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def hip(rc):
    from radiocore._internal import hip
    return hip


@pytest.fixture(scope="module")
def torch(rc):
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(torch, a, offset_floats=0):
    """The array on the device, its first element `offset_floats` floats behind an allocation's start."""
    a = np.ascontiguousarray(a)
    flat = torch.from_numpy(a.view(np.uint8).reshape(-1))
    buf = torch.empty(flat.numel() + 4 * offset_floats + 64, dtype=torch.uint8, device="cuda")
    view = buf[4 * offset_floats:4 * offset_floats + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 256 == (4 * offset_floats) % 256
    return view


class _Mix:
    """An rcfm_mix_t made straight from a case's tables."""

    def __init__(self, hip, case):
        self.hip, self.lib = hip, hip.lib()
        ip = ctypes.POINTER(ctypes.c_int32)
        chan = np.ascontiguousarray(case.chan if case.chan.size else np.zeros(1), dtype=np.int32)
        gain = np.ascontiguousarray(case.gain if case.gain.size else np.zeros((1, 2)), dtype=np.float32)
        h = _vp()
        hip.check(self.lib.rcfm_mix_create(case.M, case.bus_start.ctypes.data_as(ip), chan.ctypes.data_as(ip),
                                           gain.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), case.ch_out, ctypes.byref(h)))
        self.h = hip.Handle(h, self.lib.rcfm_mix_destroy)


def _run(hip, torch, mix, case, audio_dev, open_dev, offset_out=0, stream=None, counts=True):
    """(out [M, A, ch_out], active or None, bus_open or None) of one rcfm_mix_run; nothing around the outputs was written."""
    n = case.M * case.A * case.ch_out
    buf = torch.full((n + 8 + offset_out,), -1.0, dtype=torch.float32, device="cuda")
    out = buf[offset_out:]
    assert out.data_ptr() % 16 == (4 * offset_out) % 16
    active = torch.full((case.M + 2,), -7, dtype=torch.int32, device="cuda")
    bus_open = torch.full((case.M + 2,), 9, dtype=torch.uint8, device="cuda")
    s = hip.stream() if stream is None else _vp(stream.cuda_stream)
    hip.check(mix.lib.rcfm_mix_run(mix.h.value, case.first, case.count, case.A, case.ch_in, _vp(audio_dev.data_ptr()),
                                   _vp(open_dev.data_ptr()) if open_dev is not None else None, hip.ptr(out),
                                   hip.ptr(active) if counts else None, hip.ptr(bus_open) if counts else None, s))
    if stream is not None:
        stream.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:offset_out] == -1.0) and np.all(got[offset_out + n:] == -1.0)
    a, b = active.cpu().numpy(), bus_open.cpu().numpy()
    assert np.all(a[case.M:] == -7) and np.all(b[case.M:] == 9)
    if not counts:
        assert np.all(a == -7) and np.all(b == 9)
        return got[offset_out:offset_out + n].reshape(case.M, case.A, case.ch_out), None, None
    return got[offset_out:offset_out + n].reshape(case.M, case.A, case.ch_out), a[:case.M], b[:case.M]


def _check(case, got):
    out, active, bus_open = got
    want, want_active, want_open = case.want()
    bad = np.flatnonzero(_bits(out) != _bits(want))
    assert bad.size == 0, (case.name, bad.size, bad[:5], out.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])
    if active is not None:
        assert np.array_equal(active, want_active) and np.array_equal(bus_open, want_open), case.name


@pytest.mark.parametrize("case", mm.cases(), ids=lambda c: c.name)
def test_mix_against_model(hip, torch, case):
    """Route counts 0, 1, 15, 16, 17, 33, 100 (and 40, 64, and five routes that are all closed) in one mixer at every A of
    {1, 5, 64, 1000, 4099} and every leg combination; M = 1, 3 and 64; channels in several buses; open = NULL; a sub-range;
    NaN in the closed rows; buses of 129 .. 300 routes.  A = 4099 and A = 5 put every other row on a 4-byte boundary (the
    4-byte form), 64 and 1000 take the 16-byte form; 1000 and 4099 take several workgroups per bus; 33 .. 100 routes are up to
    seven segments, one per wave of a workgroup, and more than 128 routes take the workgroup's eight waves several rounds."""
    audio = _dev(torch, case.audio)
    opened = _dev(torch, case.open) if case.open is not None else None
    got = _run(hip, torch, _Mix(hip, case), case, audio, opened)
    _check(case, got)
    assert np.isfinite(got[0]).all()
    if case.name.startswith("sweep"):
        assert got[1][0] == 0 and got[1][-1] == 0 and not _bits(got[0][[0, -1]]).any()      # no route; all routes closed: +0


@pytest.mark.parametrize("name", ["sweep A=1000 2->2", "sweep A=1000 1->1", "sweep A=4099 1->2", "M=64", "NaN in closed rows",
                                  "long buses 1->2"])
def test_mix_bit_identity(hip, torch, name):
    """Two runs; a second stream; audio and out each one float off a 16-byte boundary; active and bus_open NULL: the same
    bits, the model's."""
    case = mm.case(name)
    mix = _Mix(hip, case)
    audio = _dev(torch, case.audio)
    opened = _dev(torch, case.open) if case.open is not None else None
    first = _run(hip, torch, mix, case, audio, opened)
    _check(case, first)
    _check(case, _run(hip, torch, mix, case, audio, opened))
    torch.cuda.synchronize()
    _check(case, _run(hip, torch, mix, case, audio, opened, stream=torch.cuda.Stream()))
    off = _dev(torch, case.audio, offset_floats=1)
    assert off.data_ptr() % 16 == 4
    _check(case, _run(hip, torch, mix, case, off, opened))
    _check(case, _run(hip, torch, mix, case, audio, opened, offset_out=1))
    _check(case, _run(hip, torch, mix, case, off, opened, offset_out=1))
    _check(case, _run(hip, torch, mix, case, audio, opened, counts=False))


def test_run_refuses_overlap_and_foreign_channels(rc, hip, torch):
    """The two refusals that read the handle -- ch_out, the host copy of the routes -- and so need a real one: nothing is
    launched."""
    lib = hip.lib()
    mixer = rc.Mixer([rc.Bus.of([3, 5]), rc.Bus([])])
    h = mixer._create(*mixer._split(((0, 8),), 8)[1][0])
    audio = torch.zeros((8, 100, 1), dtype=torch.float32, device="cuda")
    out = torch.full((2, 100, 2), -1.0, dtype=torch.float32, device="cuda")

    def run(first, count, a, o):
        return lib.rcfm_mix_run(h.value, first, count, 100, 1, _vp(a), None, _vp(o), None, None, hip.stream())
    for o in (audio.data_ptr(), audio.data_ptr() + 4 * 799, audio.data_ptr() - 4 * 399):
        assert run(0, 8, audio.data_ptr(), o) == ERR_ARG and b"overlaps" in lib.rcfm_last_error()
    for first, count in ((4, 4), (0, 5), (6, 2), (-2, 5)):
        assert run(first, count, audio.data_ptr(), out.data_ptr()) == ERR_INDEX, (first, count)
        assert b"outside [first, first + count)" in lib.rcfm_last_error()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -1.0)
    assert run(3, 3, audio.data_ptr() + 4 * 300, out.data_ptr()) == 0                      # channels 3 .. 5 alone
    torch.cuda.synchronize()
    assert not _bits(out.cpu().numpy()).any()


# ---- through the Tuner -----------------------------------------------------------------------------------------------------

import gate_model as gm  # noqa: E402


def _tables(mixer):
    start = np.concatenate([[0], np.cumsum([len(b) for b in mixer.buses])]).astype(np.int32)
    chan = np.concatenate([b.channels for b in mixer.buses] + [np.zeros(0, np.int32)])
    gain = np.concatenate([b.gains for b in mixer.buses] + [np.zeros((0, 2), np.float32)])
    return start, chan, gain


def _model(mixer, audio, mask, first=0, buses=None):
    """The model's (out, active, bus_open) for `mixer` (or its buses `buses` alone, the others empty) on audio
    [count, A, ch] of channels [first, first + count)."""
    keep = range(mixer.M) if buses is None else buses
    start = np.concatenate([[0], np.cumsum([len(b) if m in keep else 0 for m, b in enumerate(mixer.buses)])]).astype(np.int32)
    chan = np.concatenate([b.channels for m, b in enumerate(mixer.buses) if m in keep] + [np.zeros(0, np.int32)])
    gain = np.concatenate([b.gains for m, b in enumerate(mixer.buses) if m in keep] + [np.zeros((0, 2), np.float32)])
    return mm.mix(audio, None if mask is None else np.asarray(mask).astype(np.uint8), first, start, chan, gain, mixer.ch_out)


def _same(t, mixer, audio, mask, what=""):
    out, active, _ = _model(mixer, audio, mask)
    got = t.mix()
    assert got.dtype == np.float32 and got.shape == out.shape, what
    assert np.array_equal(_bits(got), _bits(out)), what
    assert np.array_equal(t.mix_active(), active), what
    return out, active


_SCENES = {}


def _scene(rc, name):
    if name not in _SCENES:
        scene = {"mixed": gm.mixed, "stereo": gm.stereo}.get(name, lambda: gm.narrow(name))()
        f_in = scene.add_to(rc.Tuner()).input_frequency
        _SCENES[name] = (scene, scene.buffers(f_in))
    return _SCENES[name]


def _narrow_mixer(rc, stereo=True):
    """Eight channels: the always-on, the across-the-edge and two more as a group spread left to right; the channel that never
    keys on a bus of its own (idle throughout); the rest 6 dB down, and channel 0 in this bus too."""
    return rc.Mixer([rc.Bus.of([0, 3, 4, 6], gain_db=[0.0, -3.0, 2.0, 0.0], pan=[-0.8, -0.2, 0.3, 0.9], name="tower"),
                     rc.Bus.of([1], name="idle"),
                     rc.Bus.of([7, 5, 2, 0], gain_db=-6.0, name="rest")], stereo=stereo)


def _gate(rc):
    return rc.FrameGate(frames=gm.FRAMES, hang=gm.HANG, lead=gm.LEAD, ramp=gm.RAMP)


def test_tuner_level_squelch(rc):
    """Behind the level squelch: mix() is the model on the run's own audio and open_mask(), and some channels are closed.
    Without a squelch every channel is open.  Before a run with a mixer mix() raises."""
    scene, xs = _scene(rc, "FM")
    t = scene.add_to(rc.Tuner(), lambda B: rc.FM(B, 800))
    mixer = _narrow_mixer(rc)
    t.set_squelch(scene.thresholds()[0])
    t.set_mix(mixer)
    with pytest.raises(RuntimeError):
        t.mix()
    for b, x in enumerate(xs[:2]):
        t.load(x)
        audio = t.run_all()
        mask = t.open_mask()
        _, active = _same(t, mixer, audio, mask, b)
        assert 0 < mask.sum() < scene.C and active[1] == 0 and not _bits(t.mix()[1]).any()
    t.set_squelch(None)
    audio = t.run_all()
    _, active = _same(t, mixer, audio, None)
    assert active.tolist() == [4, 1, 4]


def test_tuner_over_floor(rc):
    import floor_model as fm
    t = fm.tuner_setup(rc.Tuner(), lambda: rc.FM(fm.B, fm.A))
    t.set_floor(rc.NoiseFloor(fm.CELL_HZ, half=fm.HALF, guard=fm.GUARD, quantile=fm.QUANTILE))
    t.set_squelch(rc.OverFloor(fm.OVER_DB))
    mixer = rc.Mixer([rc.Bus.of([0, 1, 2, 3], pan=[-1.0, -0.3, 0.3, 1.0]), rc.Bus.of([4, 5, 6, 7], gain_db=3.0)], stereo=False)
    t.set_mix(mixer)
    for seed in (1, 2):
        t.load(fm.buffer(seed))
        audio = t.run_all()
        mask = t.open_mask()
        assert mask.tolist() == [c in fm.STATIONS for c in range(fm.C)]
        _, active = _same(t, mixer, audio, mask, seed)
        assert active.tolist() == [3, 0] and t.mix().shape == (2, fm.A, 1)


@pytest.mark.parametrize("kind", ["AM", "FM"])
def test_tuner_frame_gate_three_buffers(rc, kind):
    """Behind the frame gate, whose closed frames are exact zeros inside open rows: three buffers, stations keying on and off."""
    scene, xs = _scene(rc, kind)
    t = scene.add_to(rc.Tuner(), lambda B: getattr(rc, kind)(B, 800))
    mixer = _narrow_mixer(rc, stereo=kind == "FM")
    to, tc = scene.thresholds()
    t.set_gate(_gate(rc), open=to, close=tc)
    t.set_mix(mixer)
    seen = set()
    for b, x in enumerate(xs):
        t.load(x)
        audio = t.run_all()
        mask = t.open_mask()
        _, active = _same(t, mixer, audio, mask, (kind, b))
        seen.add(tuple(mask.tolist()))
        assert active[1] == 0
    assert len(seen) > 1                                               # the masks changed from buffer to buffer


def test_tuner_tone_squelch(rc):
    """Behind the tone squelch, on its mask: the stations of the FM scene carry tones of 100 + 20 c Hz; the even channels want
    their own tone, the odd ones a tone nobody sends."""
    scene, xs = _scene(rc, "FM")
    t = scene.add_to(rc.Tuner(), lambda B: rc.FM(B, 800))
    mixer = _narrow_mixer(rc)
    bank = rc.ToneBank([100.0 + 20.0 * c for c in range(8)] + [300.0], frame=400)
    t.set_tones(bank, want=[c if c % 2 == 0 else 8 for c in range(8)], ratio=0.3)
    t.set_mix(mixer)
    t.load(xs[0])
    audio = t.run_all()
    mask = t.open_mask()
    print("tone squelch: open", mask.astype(int).tolist())
    assert mask[0] and not mask[1::2].any()
    _same(t, mixer, audio, mask)


def test_tuner_wbfm_balance(rc):
    """Stereo channels: balance gains, stereo buses (left to left, right to right) and mono buses (gl L + gr R)."""
    scene, xs = _scene(rc, "stereo")
    for stereo in (True, False):
        t = scene.add_to(rc.Tuner(), lambda bw: rc.WBFM(bw, 12000))
        mixer = rc.Mixer([rc.Bus.of([0, 1, 2], gain_db=[0.0, -2.0, 1.0], balance=[-0.5, 0.0, 0.75]), rc.Bus.of([1], balance=1.0)],
                         stereo=stereo)
        t.set_squelch(scene.thresholds()[0])
        t.set_mix(mixer)
        t.load(xs[0])
        audio = t.run_all()
        assert audio.shape == (3, 12000, 2)
        mask = t.open_mask()
        _same(t, mixer, audio, mask, stereo)
        assert t.mix().shape == (2, 12000, 2 if stereo else 1) and mask.any()


def test_tuner_run_each_buses_per_group(rc):
    """Two launch groups (2000-sample channels with 800 samples of audio, 4000 with 1600): a handle per group, a list per bus,
    each bus as long as its group's audio; a bus across the groups is refused before anything runs."""
    scene, xs = _scene(rc, "mixed")
    t = scene.add_to(rc.Tuner(), lambda B: rc.FM(B, B * 2 // 5))
    mixer = rc.Mixer([rc.Bus.of([0, 1, 3], pan=[-0.5, 0.0, 0.5]), rc.Bus.of([5, 4], gain_db=-3.0), rc.Bus([])])
    to, tc = scene.thresholds()
    t.set_gate(_gate(rc), open=to, close=tc)
    t.set_mix(mixer)
    for b, x in enumerate(xs):
        t.load(x)
        each = t.run_each()
        mask = t.open_mask()
        low = np.stack(each[:4])                                       # [4, 800, 1]
        high = np.stack(each[4:])                                      # [2, 1600, 1]
        want_low, act_low, _ = _model(mixer, low, mask[:4], first=0, buses=[0, 2])
        want_high, act_high, _ = _model(mixer, high, mask[4:], first=4, buses=[1])
        got = t.mix()
        assert isinstance(got, list) and [g.shape for g in got] == [(800, 2), (1600, 2), (800, 2)]
        assert np.array_equal(_bits(got[0]), _bits(want_low[0])) and np.array_equal(_bits(got[1]), _bits(want_high[1]))
        assert not _bits(got[2]).any()
        assert t.mix_active().tolist() == [act_low[0], act_high[1], 0]
    t.set_mix(rc.Mixer([rc.Bus.of([3, 4])]))
    t.load(xs[0])
    with pytest.raises(ValueError, match="launch groups"):
        t.run_each()


def test_tuner_packed_buses_through_a_drain(rc):
    """run_all_packed(buses=True) through a Drain, three buffers: the rows are the buses with an open channel, the payloads the
    model's quantisation of the model's mix; no row is drained for the idle bus."""
    scene, xs = _scene(rc, "FM")
    demod = lambda B: rc.FM(B, 800)
    t, ref = scene.add_to(rc.Tuner(), demod), scene.add_to(rc.Tuner(), demod)
    mixer = _narrow_mixer(rc)
    to, tc = scene.thresholds()
    for u in (t, ref):
        u.set_gate(_gate(rc), open=to, close=tc)
    t.set_mix(mixer)
    pcm = rc.PCM("int16", 8192.0)
    drain = rc.Drain(mixer.M, (800, 2), pcm.dtype, depth=2)
    t.load(xs[0])
    with pytest.raises(ValueError):                                    # the channel rows' geometry: refused before anything runs
        t.run_all_packed(pcm, drain=rc.Drain(scene.C, (800, 1), pcm.dtype), buses=True)
    for b, x in enumerate(xs):
        ref.load(x)
        audio = ref.run_all()
        mask = ref.open_mask()
        out, active, bus_open = _model(mixer, audio, mask)
        t.load(x)
        assert t.run_all_packed(pcm, drain=drain, buses=True) is None
        with drain.next() as (index, rows):
            assert index.tolist() == np.flatnonzero(bus_open).tolist() and 1 not in index.tolist() and len(index) >= 1
            assert rows.dtype == np.int16 and rows.shape == (len(index), 800, 2)
            assert np.array_equal(np.asarray(rows), mm.pcm_s16(out[index], 8192.0)), b
        assert np.array_equal(_bits(t.mix()), _bits(out)) and np.array_equal(t.open_mask(), mask)
    # without a drain: (index, rows) of the open buses
    t.load(xs[0])
    ref.load(xs[0])
    out, _, bus_open = _model(mixer, ref.run_all(), ref.open_mask())
    index, rows = t.run_all_packed(rc.PCM("float32"), buses=True)
    assert index.tolist() == np.flatnonzero(bus_open).tolist() and np.array_equal(_bits(rows), _bits(out[index]))
    drain.close()


def test_tuner_lanes_against_one_lane(rc):
    """Lanes(depth=2): the lanes share the setting and the handle; every ticket's buses are the loop's, bit for bit."""
    scene, xs = _scene(rc, "FM")
    demod = lambda B: rc.FM(B, 800)
    loop, laned = scene.add_to(rc.Tuner(), demod), scene.add_to(rc.Tuner(), demod)
    mixer = _narrow_mixer(rc)
    to, tc = scene.thresholds()
    want = []
    for u in (loop, laned):
        u.set_gate(_gate(rc), open=to, close=tc)
        u.set_mix(mixer)
    for x in xs:
        loop.load(x)
        audio = loop.run_all()
        want.append((audio, loop.mix()))
    lanes = rc.Lanes(laned, depth=2)
    tickets = [lanes.submit(x) for x in xs]
    for b, tk in enumerate(tickets):
        audio, buses = lanes.result(tk, mix=True)
        assert np.array_equal(_bits(audio), _bits(want[b][0])) and np.array_equal(_bits(buses), _bits(want[b][1])), b
    assert lanes._tuners[1]._mix_handles is laned._mix_handles and len(laned._mix_handles) == 1
    laned.set_mix(None)
    tk = lanes.submit(xs[0])
    assert lanes.result(tk, mix=True)[1] is None


def test_tuner_growing_channel_list_and_reset(rc):
    """Routes name channel indices: a mixer over the first channels keeps working when more are added; a route to a channel
    that is not there (yet, or any more after reset()) is a ValueError."""
    scene, xs = _scene(rc, "FM")
    demod = lambda B: rc.FM(B, 800)
    order = [0, 7, 1, 2, 3, 4, 5, 6]                                   # the outermost first: the input geometry is final
    t = scene.add_to(rc.Tuner(), demod, order[:2])
    with pytest.raises(ValueError):
        t.set_mix(_narrow_mixer(rc))                                   # routes up to channel 7 of a tuner with two
    assert t._mix is None
    mixer = rc.Mixer([rc.Bus.of([0, 1], pan=[-1.0, 1.0])])
    t.set_mix(mixer)
    t.load(xs[0])
    _same(t, mixer, t.run_all(), None)
    for c in order[2:]:
        f, B = scene.chans[c]
        t.add_channel(f, B, demod(B))
        t.request_bandwidth(float(scene.n))
    t.load(xs[0])
    audio = t.run_all()
    assert audio.shape[0] == 8
    _same(t, mixer, audio, None)
    wide = _narrow_mixer(rc)
    t.set_mix(wide)                                                    # now every channel is there
    _same(t, wide, t.run_all(), None)
    with pytest.raises(ValueError):
        t.reset()
    for c in order[:2]:
        f, B = scene.chans[c]
        t.add_channel(f, B, demod(B))
        t.request_bandwidth(float(scene.n))
    t.load(xs[0])
    with pytest.raises(ValueError):
        t.run_all()


class _Trace:
    """librcfm with the names of the entry points called through it."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def test_set_mix_none_restores_the_parents_path(rc):
    """With the mixer off again the calls are those of a tuner that never had one, and so are the bits; with it on the audio
    is the same and exactly one more call is made per run."""
    scene, xs = _scene(rc, "FM")
    demod = lambda B: rc.FM(B, 800)
    plain, t = scene.add_to(rc.Tuner(), demod), scene.add_to(rc.Tuner(), demod)
    to, tc = scene.thresholds()
    for u in (plain, t):
        u.set_gate(_gate(rc), open=to, close=tc)
    t.set_mix(_narrow_mixer(rc))
    plain.load(xs[0])
    t.load(xs[0])
    assert np.array_equal(_bits(t.run_all()), _bits(plain.run_all()))  # the mixer leaves the channel audio alone
    t.set_mix(None)
    plain._lib, t._lib = _Trace(plain._lib), _Trace(t._lib)
    for x in xs[1:]:
        plain.load(x)
        t.load(x)
        assert np.array_equal(_bits(t.run_all()), _bits(plain.run_all())) and np.array_equal(t.open_mask(), plain.open_mask())
    assert t._lib.names == plain._lib.names and "rcfm_pipeline_run" in t._lib.names
    assert not [n for n in t._lib.names if "mix" in n]
    with pytest.raises(RuntimeError):
        t.mix()
    t.set_mix(_narrow_mixer(rc))
    for _ in range(2):                                                 # (the handle is made by the first run, and kept)
        t._lib.names.clear()
        plain._lib.names.clear()
        plain.run_all()
        t.run_all()
        assert t._lib.names == plain._lib.names + ["rcfm_mix_run"]
    assert len(t._mix_handles) == 1


def test_airband_mix_example():
    """examples/airband_mix.py at its --small geometry: every drained payload equals the model's quantisation, the standby bus
    is never drained, a bus is drained exactly when one of its channels is open, and the two byte counts the example reports
    are those of the rows drained and of the open channel rows."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("airband_mix", os.path.join(ROOT, "examples", "airband_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    buses, seconds = mod.run(**mod.SMALL)
    assert len(seconds) == 3 and [b.name for b in buses] == ["tower", "everything else", "standby"]
    assert any(r["drained"] for r in seconds)
    for r in seconds:
        assert r["equal"]
        assert 2 not in r["drained"] and 2 in r["idle"]
        assert sorted(r["drained"] + r["idle"]) == [0, 1, 2]
        assert [m for m in range(3) if r["active"][m] > 0] == r["drained"]
        assert r["bus_bytes"] == len(r["drained"]) * mod.AUDIO * 2 * 2 and r["channel_bytes"] == r["open_channels"] * mod.AUDIO * 2
