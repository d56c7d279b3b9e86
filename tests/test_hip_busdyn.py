"""GPU: the bus dynamics (include/rcfm.h, "bus dynamics") against tests/busdyn_model.py.

rcfm_busdyn_run: audio, bus_open_out and the state (rcfm_busdyn_state) equal the model's bit for bit over three consecutive
calls -- every operation is one float32 rounding in a stated order, so there is no tolerance.  tests/test_busdyn_model.py
shows that a kernel that fused the interpolation, ran the release in float64 or looked one block less ahead differs from the
model in 2 % of the samples or more on its burst inputs.
Through the Tuner: mix() equals the model applied to the same run's mix(dry=True) and mix_active(), buffer after buffer,
behind every kind of squelch; payloads drained with buses=True equal the model's quantisation.
"""

import ctypes

import numpy as np
import pytest

import busdyn_model as bm
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ERR_ARG = -4
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


class _Dyn:
    """An rcfm_busdyn_t made straight from a model's Params."""

    def __init__(self, hip, p, A_max):
        from radiocore.tools import busdyn
        self.hip, self.lib, self.p = hip, hip.lib(), p
        self.h = busdyn.create(p.M, p.ch, p.L, A_max, p.c, p.k, *(p.tables() if p.key is not None else ()))

    def state(self):
        p = self.p
        tail, h, hang = np.full((p.M, p.L, p.ch), -3.0, np.float32), np.full(p.M, -3.0, np.float32), np.full(p.M, -3, np.int32)
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        self.hip.check(self.lib.rcfm_busdyn_state(self.h.value, tail.ctypes.data_as(fp), h.ctypes.data_as(fp), hang.ctypes.data_as(ip)))
        return tail, h, hang


def _run(hip, torch, dyn, x, opened, offset_in=0, offset_out=0, stream=None, open_out=True):
    """(out [M, A, ch], bus_open_out or None) of one rcfm_busdyn_run; nothing around the outputs was written."""
    M, A, ch = x.shape
    n = M * A * ch
    x_dev = _dev(torch, x, offset_floats=offset_in)
    open_dev = _dev(torch, opened) if opened is not None else None
    buf = torch.full((n + 8 + offset_out,), -1.0, dtype=torch.float32, device="cuda")
    out = buf[offset_out:]
    assert out.data_ptr() % 16 == (4 * offset_out) % 16
    flags = torch.full((M + 2,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = hip.stream() if stream is None else _vp(stream.cuda_stream)
    hip.check(dyn.lib.rcfm_busdyn_run(dyn.h.value, A, _vp(x_dev.data_ptr()), _vp(open_dev.data_ptr()) if open_dev is not None else None,
                                      hip.ptr(out), hip.ptr(flags) if open_out else None, s))
    if stream is not None:
        stream.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[:offset_out] == -1.0) and np.all(got[offset_out + n:] == -1.0)
    f = flags.cpu().numpy()
    assert np.all(f[M:] == 9)
    if not open_out:
        assert np.all(f == 9)
    return got[offset_out:offset_out + n].reshape(M, A, ch), f[:M] if open_out else None


def _check(name, q, got, want, dyn=None):
    out, open_out = got
    w_out, w_open, w_state = want
    bad = np.flatnonzero(_bits(out) != _bits(w_out))
    assert bad.size == 0, (name, q, bad.size, bad[:5], out.reshape(-1)[bad[:5]], w_out.reshape(-1)[bad[:5]])
    if open_out is not None:
        assert np.array_equal(open_out, w_open), (name, q)
    if dyn is not None:
        tail, h, hang = dyn.state()
        assert np.array_equal(_bits(tail), _bits(w_state.tail)), (name, q)
        assert np.array_equal(_bits(h), _bits(w_state.h)) and np.array_equal(hang, w_state.hang), (name, q, h, w_state.h, hang, w_state.hang)


def _sequence(hip, torch, case, A_max=None, **kw):
    dyn = _Dyn(hip, case.p, case.A if A_max is None else A_max)
    for q, (x, o, want) in enumerate(zip(case.x, case.open, case.want())):
        _check(case.name, q, _run(hip, torch, dyn, x, o, **kw), want, dyn)
    return dyn


@pytest.mark.parametrize("case", bm.cases(), ids=lambda c: c.name)
def test_busdyn_against_model(hip, torch, case):
    """Three consecutive calls per case: A of {1, 5, 63, 64, 65, 1000, 4099} at L of {8, 64, 100}, both leg counts, with and
    without duck tables, every bus a burst, steady over-level noise, noise below the ceiling or +0 in turn; L = 2048 at A =
    1000 (A < L); M = 1, 3 and 64; every input kind on all buses at once; hold = 0; a key chain; bus_open_in = NULL.  A = 5,
    63, 65 and 4099 with one leg, and L = 100 with one leg at some A, take the 4-byte loads of the peaks, the others the
    16-byte ones; A = 1000 and 4099 take several workgroups per bus in the apply."""
    _sequence(hip, torch, case)
    for out, _, _ in case.want():
        assert np.all(np.abs(out) <= case.p.c)


@pytest.mark.parametrize("name", ["sweep A=1000 L=64 ch=2", "sweep A=4099 L=100 ch=1", "sweep A=65 L=8 ch=2", "M=64 ch=2", "key chain",
                                  "L=2048 ch=1"])
def test_busdyn_bit_identity(hip, torch, name):
    """Two handles run from equal state; a second stream; in and out each one float off a 16-byte boundary; bus_open_out NULL;
    a handle made for longer rows: the same bits and the same state, the model's."""
    case = bm.case(name)
    _sequence(hip, torch, case)
    _sequence(hip, torch, case)
    torch.cuda.synchronize()
    _sequence(hip, torch, case, stream=torch.cuda.Stream())
    _sequence(hip, torch, case, offset_in=1)
    _sequence(hip, torch, case, offset_out=1)
    _sequence(hip, torch, case, offset_in=1, offset_out=1)
    _sequence(hip, torch, case, open_out=False)
    _sequence(hip, torch, case, A_max=case.A + 137)


def test_busdyn_reset_and_fence(hip, torch):
    """reset puts the state back to what create left; with the fence on, calls that alternate between two streams give the
    sequence's bits."""
    case = bm.case("sweep A=1000 L=64 ch=2")
    dyn = _sequence(hip, torch, case)
    assert np.any(dyn.state()[0] != 0)
    hip.check(dyn.lib.rcfm_busdyn_reset(dyn.h.value, hip.stream()))
    tail, h, hang = dyn.state()
    assert not _bits(tail).any() and np.all(h == 1.0) and not hang.any()
    for q, (x, o, want) in enumerate(zip(case.x, case.open, case.want())):
        _check(case.name, q, _run(hip, torch, dyn, x, o), want, dyn)
    fenced = _Dyn(hip, case.p, case.A)
    hip.check(fenced.lib.rcfm_busdyn_set_fence(fenced.h.value, 1))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    x_dev = [_dev(torch, x) for x in case.x]
    o_dev = [_dev(torch, o) for o in case.open]
    outs = [torch.empty(case.x[0].shape, dtype=torch.float32, device="cuda") for _ in case.x]
    torch.cuda.synchronize()
    for q in range(3):
        hip.check(fenced.lib.rcfm_busdyn_run(fenced.h.value, case.A, _vp(x_dev[q].data_ptr()), _vp(o_dev[q].data_ptr()),
                                             hip.ptr(outs[q]), None, _vp(streams[q % 2].cuda_stream)))
    torch.cuda.synchronize()
    for q, want in enumerate(case.want()):
        assert np.array_equal(_bits(outs[q].cpu().numpy()), _bits(want[0])), q
    hip.check(fenced.lib.rcfm_busdyn_set_fence(fenced.h.value, 0))


def test_run_refuses_what_needs_a_handle(hip, torch):
    """A above A_max and partly overlapping buffers are refused on the handle's figures: nothing is launched."""
    p = bm.Params(2, 2, 8, 0.5, 0.5)
    dyn = _Dyn(hip, p, 100)
    lib = dyn.lib
    x = torch.ones((2, 101, 2), dtype=torch.float32, device="cuda")
    out = torch.full((2, 101, 2), -1.0, dtype=torch.float32, device="cuda")

    def run(A, i, o):
        return lib.rcfm_busdyn_run(dyn.h.value, A, _vp(i), None, _vp(o), None, hip.stream())
    assert run(101, x.data_ptr(), out.data_ptr()) == ERR_ARG and b"A_max" in lib.rcfm_last_error()
    for o in (x.data_ptr(), x.data_ptr() + 4 * 399, x.data_ptr() - 4 * 399):
        assert run(100, x.data_ptr(), o) == ERR_ARG and b"overlaps" in lib.rcfm_last_error()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -1.0)
    tail, h, hang = dyn.state()
    assert not _bits(tail).any() and np.all(h == 1.0)
    assert run(100, x.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(-1)
    assert np.all(np.abs(got[:400]) <= 0.5) and np.all(got[400:] == -1.0)


# ---- through the Tuner -----------------------------------------------------------------------------------------------------

import gate_model as gm  # noqa: E402
from test_hip_mix import _gate, _narrow_mixer, _scene  # noqa: E402


class _Follow:
    """The model beside a Tuner: Params from the Limiter and the ducks at the rate A, the state carried from buffer to buffer;
    step() checks the tuner's last run against it."""

    def __init__(self, rc, mixer, limiter, ducks, A):
        from radiocore.tools import busdyn
        self.L, c, k = limiter.discretise(A)
        tables = (None,) * 4
        if ducks:
            key, per = busdyn.resolve_ducks(ducks, mixer.buses)
            d = [x.discretise(A, self.L) if x is not None else (1.0, 0.0, 0) for x in per]
            tables = (key, [v[0] for v in d], [v[1] for v in d], [v[2] for v in d])
        self.p = bm.Params(mixer.M, mixer.ch_out, self.L, c, k, *tables)
        self.st = bm.State(self.p)
        self.engaged = False

    def model(self, dry, active):
        out, open_out, self.st = bm.run(self.p, self.st, dry, (np.asarray(active) > 0).astype(np.uint8))
        self.engaged = self.engaged or bool(np.any(self.st.h < 1.0))
        return out, open_out

    def step(self, t, what=""):
        dry = t.mix(dry=True)
        out, open_out = self.model(dry, t.mix_active())
        got = t.mix()
        assert got.dtype == np.float32 and got.shape == out.shape, what
        assert np.array_equal(_bits(got), _bits(out)), what
        assert np.all(np.abs(got) <= self.p.c) and t.bus_delay() == [self.L], what
        return out, open_out


LIMITER = dict(ceiling_db=-40.0, lookahead=0.02, release=0.1)          # A = 800: blocks of 16 samples, 50 per buffer


def test_tuner_level_squelch(rc):
    """Behind the level squelch, three buffers: mix() is the model on the run's own mix(dry=True) and mix_active(); the limiter
    has something to do, and the channel audio is what it is without the stage."""
    scene, xs = _scene(rc, "FM")
    t, plain = scene.add_to(rc.Tuner(), lambda B: rc.FM(B, 800)), scene.add_to(rc.Tuner(), lambda B: rc.FM(B, 800))
    mixer = _narrow_mixer(rc)
    lim, ducks = rc.Limiter(**LIMITER), {"rest": rc.Duck("tower", depth_db=-9.0, threshold_db=-60.0, hold=0.05)}
    for u in (t, plain):
        u.set_squelch(scene.thresholds()[0])
        u.set_mix(mixer)
    t.set_bus_dynamics(lim, ducks)
    f = _Follow(rc, mixer, lim, ducks, 800)
    assert f.L == 16
    for b, x in enumerate(xs):
        t.load(x)
        plain.load(x)
        audio = t.run_all()
        assert np.array_equal(_bits(audio), _bits(plain.run_all())) and np.array_equal(_bits(t.mix(dry=True)), _bits(plain.mix()))
        f.step(t, b)
    assert f.engaged
    t.reset_states()
    f.st = bm.State(f.p)
    t.load(xs[0])
    t.run_all()
    f.step(t, "after reset_states")


@pytest.mark.parametrize("kind", ["AM", "FM"])
def test_tuner_frame_gate_three_buffers(rc, kind):
    """Behind the frame gate, whose closed frames are exact zeros inside open rows; mono buses for AM."""
    scene, xs = _scene(rc, kind)
    t = scene.add_to(rc.Tuner(), lambda B: getattr(rc, kind)(B, 800))
    mixer = _narrow_mixer(rc, stereo=kind == "FM")
    to, tc = scene.thresholds()
    t.set_gate(_gate(rc), open=to, close=tc)
    t.set_mix(mixer)
    lim = rc.Limiter(**LIMITER)
    t.set_bus_dynamics(lim)
    f = _Follow(rc, mixer, lim, None, 800)
    for b, x in enumerate(xs):
        t.load(x)
        t.run_all()
        f.step(t, (kind, b))
    assert f.engaged


def test_tuner_wbfm_stereo_buses(rc):
    """Stereo channels on stereo buses, 12 000 samples of audio: blocks of 96."""
    scene, xs = _scene(rc, "stereo")
    t = scene.add_to(rc.Tuner(), lambda bw: rc.WBFM(bw, 12000))
    mixer = rc.Mixer([rc.Bus.of([0, 1, 2], gain_db=[0.0, -2.0, 1.0], balance=[-0.5, 0.0, 0.75], name="all"),
                      rc.Bus.of([1], balance=1.0, name="one")])
    t.set_squelch(scene.thresholds()[0])
    t.set_mix(mixer)
    lim, ducks = rc.Limiter(ceiling_db=-80.0), {"all": rc.Duck("one", depth_db=-6.0, threshold_db=-140.0, hold=0.1)}
    t.set_bus_dynamics(lim, ducks)
    f = _Follow(rc, mixer, lim, ducks, 12000)
    assert f.L == 96
    for b, x in enumerate(xs):
        t.load(x)
        assert t.run_all().shape == (3, 12000, 2)
        f.step(t, b)
        assert t.mix().shape == (2, 12000, 2)
    assert f.engaged


def test_tuner_run_each_two_groups(rc):
    """Two launch groups (800 and 1600 samples of audio): a handle per group at the group's rate, every bus in each; a duck
    inside a group works, one across the groups is refused before anything runs."""
    scene, xs = _scene(rc, "mixed")
    t = scene.add_to(rc.Tuner(), lambda B: rc.FM(B, B * 2 // 5))
    mixer = rc.Mixer([rc.Bus.of([0, 1, 3], pan=[-0.5, 0.0, 0.5]), rc.Bus.of([5, 4], gain_db=-3.0), rc.Bus.of([2, 0])])
    to, tc = scene.thresholds()
    t.set_gate(_gate(rc), open=to, close=tc)
    t.set_mix(mixer)
    lim, ducks = rc.Limiter(**LIMITER), {2: rc.Duck(0, threshold_db=-60.0, hold=0.03)}
    t.set_bus_dynamics(lim, ducks)
    low, high = _Follow(rc, mixer, lim, ducks, 800), _Follow(rc, mixer, lim, ducks, 1600)
    assert (low.L, high.L) == (16, 32)
    for b, x in enumerate(xs):
        t.load(x)
        t.run_each()
        dry, got, active = t.mix(dry=True), t.mix(), t.mix_active()
        assert [g.shape for g in got] == [(800, 2), (1600, 2), (800, 2)] and t.bus_delay() == [16, 32]
        # group 0 owns the buses 0 and 2, group 1 the bus 1; the others are rows of +0 there, with nothing open
        want_low, _ = low.model(np.stack([dry[0], np.zeros_like(dry[0]), dry[2]]), [active[0], 0, active[2]])
        want_high, _ = high.model(np.stack([np.zeros_like(dry[1]), dry[1], np.zeros_like(dry[1])]), [0, active[1], 0])
        for m, want in ((0, want_low[0]), (1, want_high[1]), (2, want_low[2])):
            assert np.array_equal(_bits(got[m]), _bits(want)), (b, m)
    assert low.engaged and high.engaged
    t.set_bus_dynamics(lim, {1: rc.Duck(0)})
    t.load(xs[0])
    with pytest.raises(ValueError, match="launch group"):
        t.run_each()


def test_tuner_packed_buses_through_a_drain(rc):
    """run_all_packed(buses=True) through a Drain: the rows are the buses bus_open_out names, the payloads the numpy
    quantisation of the model.  After the stations, silence: a bus that went idle is drained exactly once more, while its
    tail comes out, and not after that."""
    scene, xs = _scene(rc, "FM")
    t = scene.add_to(rc.Tuner(), lambda B: rc.FM(B, 800))
    mixer = _narrow_mixer(rc)
    t.set_squelch(scene.thresholds()[0])
    t.set_mix(mixer)
    lim = rc.Limiter(**LIMITER)
    t.set_bus_dynamics(lim)
    f = _Follow(rc, mixer, lim, None, 800)
    pcm = rc.PCM("int16", 8192.0 * 64)
    drain = rc.Drain(mixer.M, (800, 2), pcm.dtype, depth=2)
    silence = np.zeros(scene.n, np.complex64)
    history = []
    for b, x in enumerate(list(xs) + [silence] * 3):
        t.load(x)
        assert t.run_all_packed(pcm, drain=drain, buses=True) is None
        active = t.mix_active()
        out, open_out = f.model(t.mix(dry=True), active)
        with drain.next() as (index, rows):
            assert index.tolist() == np.flatnonzero(open_out).tolist(), b
            assert rows.dtype == np.int16 and rows.shape == (len(index), 800, 2)
            assert np.array_equal(np.asarray(rows), bm.pcm_s16(out[index], pcm.gain)), b
            history.append((active.copy(), set(index.tolist())))
        assert np.array_equal(_bits(t.mix()), _bits(out))
    (a3, d3), (a4, d4), (a5, d5) = history[3:]
    assert history[2][0][0] > 0 and 0 in history[2][1]                  # the tower bus was open in the last buffer with stations
    assert not a3.any() and not a4.any() and not a5.any()               # silence: no channel is open
    assert 0 in d3 and not d4 and not d5                                # one more row, the tail; none after that
    assert 1 not in set().union(*[d for _, d in history])               # the bus that never had an open channel: never drained
    drain.close()


def test_tuner_lanes_against_one_lane(rc):
    """Lanes(depth=2): the lanes share the setting, the handle and its state behind a fence; every ticket's buses are the
    loop's, bit for bit."""
    scene, xs = _scene(rc, "FM")
    demod = lambda B: rc.FM(B, 800)
    loop, laned = scene.add_to(rc.Tuner(), demod), scene.add_to(rc.Tuner(), demod)
    mixer = _narrow_mixer(rc)
    to, tc = scene.thresholds()
    lim, ducks = rc.Limiter(**LIMITER), {"rest": rc.Duck("tower", threshold_db=-60.0, hold=0.05)}
    want = []
    for u in (loop, laned):
        u.set_gate(_gate(rc), open=to, close=tc)
        u.set_mix(mixer)
        u.set_bus_dynamics(lim, ducks)
    for x in list(xs) + list(xs):
        loop.load(x)
        audio = loop.run_all()
        want.append((audio, loop.mix()))
    lanes = rc.Lanes(laned, depth=2)
    tickets = [lanes.submit(x) for x in list(xs) + list(xs)]
    for b, tk in enumerate(tickets):
        audio, buses = lanes.result(tk, mix=True)
        assert np.array_equal(_bits(audio), _bits(want[b][0])) and np.array_equal(_bits(buses), _bits(want[b][1])), b
    assert lanes._tuners[1]._busdyn_handles is laned._busdyn_handles and len(laned._busdyn_handles) == 1
    assert not np.array_equal(_bits(want[0][1]), _bits(want[3][1]))        # the state carried over: the same buffer, other bits


def test_tuner_growing_channel_list_keeps_the_state(rc):
    """Channels are added between buffers: the mixer's tables are made again, the dynamics' handle and state stay, since the
    audio length stays."""
    scene, xs = _scene(rc, "FM")
    demod = lambda B: rc.FM(B, 800)
    order = [0, 7, 1, 2, 3, 4, 5, 6]                                   # the outermost first: the input geometry is final
    t = scene.add_to(rc.Tuner(), demod, order[:2])
    mixer = rc.Mixer([rc.Bus.of([0, 1], pan=[-1.0, 1.0]), rc.Bus.of([1, 0], gain_db=-3.0)])
    t.set_mix(mixer)
    lim = rc.Limiter(**LIMITER)
    t.set_bus_dynamics(lim, {1: rc.Duck(0, threshold_db=-60.0)})
    f = _Follow(rc, mixer, lim, {1: rc.Duck(0, threshold_db=-60.0)}, 800)
    t.load(xs[0])
    t.run_all()
    f.step(t, "two channels")
    handle = list(t._busdyn_handles.values())[0][1][0][1]
    for c in order[2:]:
        fc, B = scene.chans[c]
        t.add_channel(fc, B, demod(B))
        t.request_bandwidth(float(scene.n))
    t.load(xs[1])
    assert t.run_all().shape[0] == 8
    f.step(t, "eight channels")                                        # from the state the first buffer left
    assert list(t._busdyn_handles.values())[0][1][0][1] is handle and f.engaged
    with pytest.raises(ValueError):
        t.reset()
    assert not t._busdyn_handles


class _Trace:
    """librcfm with the names of the entry points called through it."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def test_set_bus_dynamics_off_restores_the_parents_path(rc):
    """With the stage off again the calls and the bits are those of a tuner that never had it; with it on the dry rows are
    the same and exactly one more call is made per run."""
    scene, xs = _scene(rc, "FM")
    demod = lambda B: rc.FM(B, 800)
    plain, t = scene.add_to(rc.Tuner(), demod), scene.add_to(rc.Tuner(), demod)
    to, tc = scene.thresholds()
    for u in (plain, t):
        u.set_gate(_gate(rc), open=to, close=tc)
        u.set_mix(_narrow_mixer(rc))
    t.set_bus_dynamics(rc.Limiter(**LIMITER))
    plain.load(xs[0])
    t.load(xs[0])
    assert np.array_equal(_bits(t.run_all()), _bits(plain.run_all())) and np.array_equal(_bits(t.mix(dry=True)), _bits(plain.mix()))
    assert not np.array_equal(_bits(t.mix()), _bits(plain.mix()))
    t.set_bus_dynamics()
    plain._lib, t._lib = _Trace(plain._lib), _Trace(t._lib)
    for x in xs[1:]:
        plain.load(x)
        t.load(x)
        assert np.array_equal(_bits(t.run_all()), _bits(plain.run_all())) and np.array_equal(_bits(t.mix()), _bits(plain.mix()))
        assert np.array_equal(_bits(t.mix(dry=True)), _bits(plain.mix())) and t.bus_delay() == [0]
    assert t._lib.names == plain._lib.names and "rcfm_mix_run" in t._lib.names
    assert not [n for n in t._lib.names if "busdyn" in n]
    t.set_bus_dynamics(rc.Limiter(**LIMITER))
    for _ in range(2):                                                 # (the handle is made by the first run, and kept)
        t._lib.names.clear()
        plain._lib.names.clear()
        plain.run_all()
        t.run_all()
        assert t._lib.names == plain._lib.names + ["rcfm_busdyn_run"]
    assert len(t._busdyn_handles) == 1


def test_airband_mix_limited_example():
    """examples/airband_mix_limited.py at its --small geometry: four stations at once on one bus clip in the int16 payload
    without the limiter and do not with it, and the rest bus is turned down while the tower bus talks."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("airband_mix_limited", os.path.join(ROOT, "examples", "airband_mix_limited.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.run(**mod.SMALL)
    assert r["plain"]["at_full_scale"] > 0 and r["plain"]["peak"] == 32767
    assert r["limited"]["at_full_scale"] == 0 and 0 < r["limited"]["peak"] < 32767
    assert r["rest_level_talking"] < 0.5 * r["rest_level_quiet"]
