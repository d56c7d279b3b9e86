"""CPU: the whole sequence of ABI calls the Tuner makes with every optional stage on at once -- squelch, tone bank and tone
squelch, audio filter, IQ balance, blanker, retune, shard, lanes, chunked and packed runs, kernel options, and on a third
tuner the stages that carry state behind a fence (frame gate over the noise floor, audio filter, mixer, bus dynamics: through
a lane, across a growing channel list, reset_states() and reset()) -- pinned call by call against a literal list.  The library
is the counting stand-in of tests/test_am.py; no device is used.  The list is what the library sees: a change of the Tuner
that leaves behaviour alone leaves this test alone.

The second test is the invariant behind the list: every handle of a family with a fence is armed by _arm_state_fence(), every
handle of a family with a reset is reset by reset_states(), and reset() empties every carried cache -- the families read
from hip.SIGNATURES, so a stage that is added without registering its cache fails here."""

import ctypes
import re

import numpy as np
import pytest

from test_am import _CountingLib, _FakeTensor, _FakeTorch

REF, PTR = "<ref>", "<ptr>"


class _Tensor(_FakeTensor):
    dtype = "f32"

    def is_contiguous(self):
        return True

    def numel(self):
        return int(np.prod(self.shape))

    def data_ptr(self):
        return 0x100000


class _Torch(_FakeTorch):
    Tensor = _Tensor
    uint8, int16, int32, int64, float64 = "u8", "i16", "i32", "i64", "f64"

    @staticmethod
    def cat(tensors):
        return tensors[0]


def _norm(a):
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, ctypes.Array):
        return list(a)
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    return PTR if isinstance(a, ctypes._Pointer) else REF


def _trace(fake, start=0):
    return [(name,) + tuple(_norm(a) for a in args) for name, args in fake.calls[start:]]


def _names(fake, start):
    return [name for name, _ in fake.calls[start:]]


def _neither(tuner, mask=True, tones=True):
    for call, gone in ((tuner.open_mask, mask), (tuner.tone_power, tones)):
        if gone:
            with pytest.raises(RuntimeError):
                call()
        else:
            call()


@pytest.fixture()
def fake(monkeypatch):
    from radiocore._internal import hip
    lib = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: lib)
    monkeypatch.setattr(hip, "torch", lambda: _Torch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _Tensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _Tensor(x.shape if hasattr(x, "shape") else (len(x),)))
    monkeypatch.setattr(hip, "to_host", lambda x: x)
    return lib


def _scenario(fake):
    """Drives the tuners; returns the index into fake.calls where the last part (every stage off) begins, and the tuners."""
    import radiocore as rc
    from radiocore.tools import audiofilter as af, tones
    B, A, N = 12500, 8000, 600000
    x = np.zeros(N, np.complex64)

    # ---- mixed groups: two FM, two AM, every stage set before the first load
    t = rc.Tuner()
    for i in range(4):
        t.add_channel(446.0e6 + float(B) * i, B, (rc.FM if i < 2 else rc.AM)(B, A))
    t.request_bandwidth(float(N))
    _neither(t)
    bank = rc.ToneBank(tones.CTCSS)
    t.set_tones(bank, want=[88.5, None, -1, 38], ratio=0.01)
    t.set_audio_filter(af.VOICE_NFM, channels=[True, False, True, True])
    t.set_squelch(1e-3)
    t.set_iq_balance("auto", dc_notch=2)
    t.set_blanker(rc.NoiseBlanker())
    t.retune(3)
    _neither(t)
    t.load(x)
    assert len(t.run_each()) == 4
    t.tone_power()

    # ---- a lane: its own tuner and blanker handles (and scratch: it loads a device tensor), the shared filter handle
    lane = t._lane_clone()
    t._arm_state_fence()
    lane.load(_Tensor((N,)))
    lane._run_each_device()
    assert lane._afilt_handles is t._afilt_handles and lane._state_owner is t._state_owner
    assert lane._handle is not t._handle and lane._blank_handles[N][1] is not t._blank_handles[N][1]
    t.set_squelch([1e-3, 2e-3, 3e-3, 4e-3])
    _neither(t, tones=False)                 # the masks of the last run are gone, its tone powers are not
    t.retune([0, -1, 0, 2])
    t.set_iq_balance(0.01 + 0.02j)
    t.set_blanker(rc.NoiseBlanker(threshold_db=10.0), in_place=True)
    t.set_audio_filter(af.VOICE_NFM)
    lane._sync_lane(t)
    lane.load(_Tensor((N,)))
    lane._run_each_device()
    lane.tone_power()
    t.set_tones(bank, want=8, ratio=[0.01, 0.02, 0.03, 0.04])
    _neither(t)
    lane._sync_lane(t)
    _neither(lane)
    lane.load(x)
    lane._run_each_device()

    # ---- a shard
    t.shard(1, 2)
    t.load(x)
    assert len(t.run_each()) == 2
    t.load(x, whole=True)
    t.reset_states()

    # ---- one class for all channels
    u = rc.Tuner(cuda=True)
    for i in range(4):
        u.add_channel(446.0e6 + float(B) * i, B, rc.MFM(B, A))
    u.request_bandwidth(float(N))
    u.set_tones(bank, want=8, ratio=0.01)
    u.set_audio_filter(af.VOICE_NFM)
    u.set_squelch(1e-3)
    u.set_blanker(rc.NoiseBlanker())
    u.load(x)
    assert u.run_all(numpy_output=False).shape == (4, A, 1)
    u.tone_power(numpy_output=False)
    u.run_all(chunk=2)                          # a second batched handle, bound to the first one's state
    assert len(u.run_all_packed(rc.PCM("int16"), numpy_output=False)) == 3
    u.set_kernel_options(fused_tiles=False)
    u.run_all()
    u.shard(0, 0)
    assert u.run_all(numpy_output=False).shape == (0, A, 1)       # launched with count 0, no gates
    _neither(u)
    u.add_channel(446.0e6 + float(B) * 4, B, rc.MFM(B, A))       # the filter's states move into a longer handle
    u.shard(0, 5)
    u.set_tones(bank, want=8, ratio=0.01)
    u.load(x)
    assert u.run_all(numpy_output=False).shape == (5, A, 1)

    # ---- the stages that carry state behind a fence: frame gate over the noise floor, audio filter, mixer, bus dynamics
    v = rc.Tuner()
    for i in range(4):
        v.add_channel(446.0e6 + float(B) * i, B, rc.MFM(B, A))
    v.request_bandwidth(float(N))
    v.set_floor(rc.NoiseFloor(1000.0, half=40, guard=8, quantile=0.25))
    v.set_gate(rc.FrameGate(frames=50), open=rc.OverFloor(10))
    v.set_audio_filter(af.VOICE_NFM)
    v.set_mix(rc.Mixer([rc.Bus.of([1, 3], name="tower"), rc.Bus.of([0, 2], gain_db=-6.0, name="rest")]))
    v.set_bus_dynamics(rc.Limiter(), ducks={"rest": rc.Duck("tower")})
    v.load(x)
    v.run_all()
    vlane = v._lane_clone()
    v._arm_state_fence()                        # demodulators, audio filter, gate, floor, bus dynamics
    vlane.load(_Tensor((N,)))
    vlane._run_all_device()
    for name in ("_afilt_handles", "_gate_handles", "_floor_handles", "_mix_handles", "_busdyn_handles"):
        assert getattr(vlane, name) is getattr(v, name) and len(getattr(v, name)) == 1
    v.set_bus_dynamics(rc.Limiter(lookahead=0.002))      # new settings: the lane makes the handle, behind the fence at once
    vlane._sync_lane(v)
    vlane.load(_Tensor((N,)))
    vlane._run_each_device()
    v.add_channel(446.0e6 + float(B) * 4, B, rc.MFM(B, A))       # the filter's and the gate's states move into longer handles
    v.request_bandwidth(float(N))
    v.load(x)
    v.run_all()
    vlane._sync_lane(v)
    vlane.load(_Tensor((N,)))
    vlane._run_all_device()
    v.reset_states()
    with pytest.raises(ValueError):
        v.reset()                               # (min() of nothing, like the reference: the caches have gone by then)
    assert not (v._afilt_handles or v._gate_handles or v._floor_handles or v._mix_handles or v._busdyn_handles)
    assert v._floor_out is None

    # ---- every stage off
    u.set_tones(None)
    u.set_audio_filter(None)
    u.set_squelch(None)
    u.set_iq_balance(None)
    u.set_blanker(None)
    _neither(u)
    off = len(fake.calls)
    u.load(x)
    u.run_all()
    _neither(u)
    return off, (t, lane, u, bank, v, vlane)


def test_the_call_sequence_of_every_stage_at_once(fake):
    off, alive = _scenario(fake)         # (the trace ends before the tuners go: what is destroyed in between is part of it)
    assert _names(fake, off) == ["rcfm_tuner_load", "rcfm_pipeline_run"]
    got = _trace(fake)
    for i, (g, w) in enumerate(zip(got, EXPECTED)):
        assert g == w, (i, g, w)
    assert len(got) == len(EXPECTED)


def _handles(fake, suffix, start=0):
    """{family: [handle, ..]} of the calls rcfm_<family><suffix> since `start`: the handle rcfm_*_create handed out, else the
    first argument."""
    out = {}
    for name, args in fake.calls[start:]:
        m = re.fullmatch(r"rcfm_(\w+?)" + suffix, name)
        if m:
            out.setdefault(m.group(1), []).append(args[-1]._obj.value if suffix == "_create" else _norm(args[0]))
    return out


def test_every_carried_handle_is_fenced_reset_and_dropped(fake):
    """The invariant the registry of carried caches keeps.  The families come from the ABI's own table: a stage that adds
    rcfm_x_create and rcfm_x_set_fence (or rcfm_x_reset) must be turned on below -- and then fails here unless its cache
    is registered with the Tuner."""
    import radiocore as rc
    from radiocore._internal import hip
    from radiocore.tools import audiofilter as af, tones
    created = {m.group(1) for m in (re.fullmatch(r"rcfm_(\w+)_create", name) for name in hip.SIGNATURES) if m}
    fenced = {f for f in created if "rcfm_%s_set_fence" % f in hip.SIGNATURES}
    resettable = {f for f in created if "rcfm_%s_reset" % f in hip.SIGNATURES}
    assert {"audio_filter", "gate", "floor", "busdyn"} <= fenced and fenced <= resettable

    # every stage on, two launch groups (two bandwidths) with a bus each and a duck inside the first
    A, N = 8000, 600000
    t = rc.Tuner()
    for i in range(4):
        t.add_channel(446.0e6 + 12500.0 * i, 12500, rc.MFM(12500, A))
    for i in range(2):
        t.add_channel(446.0e6 + 12500.0 * 4 + 25000.0 * i + 6250.0, 25000, rc.MFM(25000, A))
    t.request_bandwidth(float(N))
    t.set_tones(rc.ToneBank(tones.CTCSS), want=8, ratio=0.01)
    t.set_audio_filter(af.VOICE_NFM)
    t.set_iq_balance("auto")
    t.set_blanker(rc.NoiseBlanker())
    t.set_floor(rc.NoiseFloor(1000.0, half=40, guard=8, quantile=0.25))
    t.set_gate(rc.FrameGate(frames=50), open=rc.OverFloor(10))
    t.set_mix(rc.Mixer([rc.Bus.of([1, 3], name="tower"), rc.Bus.of([0, 2], name="rest"), rc.Bus.of([4, 5], name="wide")]))
    t.set_bus_dynamics(rc.Limiter(), ducks={"rest": rc.Duck("tower")})
    t.load(np.zeros(N, np.complex64))
    t.run_each()
    made = _handles(fake, "_create")
    assert not _handles(fake, "_destroy")
    for family in fenced | resettable:
        assert made.get(family), "no %s handle was made: turn the stage on in this test" % family
    assert len(made["busdyn"]) == 2

    mark = len(fake.calls)
    t._arm_state_fence()
    armed = _handles(fake, "_set_fence", mark)
    assert {f: sorted(armed.get(f, [])) for f in fenced} == {f: sorted(made[f]) for f in fenced}
    assert all(args[1] == 1 for name, args in fake.calls[mark:] if name.endswith("_set_fence"))

    mark = len(fake.calls)
    t.reset_states()
    rested = _handles(fake, "_reset", mark)
    assert {f: sorted(rested.get(f, [])) for f in resettable} == {f: sorted(made[f]) for f in resettable}

    mark = len(fake.calls)
    with pytest.raises(ValueError):
        t.reset()                               # (min() of nothing, like the reference: the caches have gone by then)
    assert t._carried and not any(t._carried.values()) and t._floor_out is None
    gone = _handles(fake, "_destroy", mark)
    assert {f: sorted(gone.get(f, [])) for f in fenced | resettable} == {f: sorted(made[f]) for f in fenced | resettable}


# Handles are 0x1000 + the number of calls so far (4097 = the tone bank's, 4098 = the first tuner's ...); 1048576 = 0x100000 is
# every device array's address, so `+ 4 * first` (thresholds, wanted tones, ratios) and `+ first` (the filter's selection) show.
EXPECTED = [
    # mixed groups: set_tones makes the bank's handle, the first load the tuner's and the blanker's
    ('rcfm_tone_bank_create', 39, PTR, 8000, PTR, REF),
    ('rcfm_tuner_create', 600000, 4, [18747, 6247, -6253, -18753], [12500, 12500, 12500, 12500], REF),
    ('rcfm_tuner_set_iq_balance', 4098, 2, 0.0, 0.0, 2),
    ('rcfm_blanker_create', 600000, 4096, 4, 0, 15.848931924611133, 1, PTR, 1, REF),
    ('rcfm_blanker_run', 4100, 0, 600000, None, None, None, None),
    ('rcfm_tuner_load', 4098, None, None),
    ('rcfm_demod_create', 0, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_pipeline_run', 4098, 4103, 0, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_create', 4, 1, 5, PTR, REF),
    ('rcfm_audio_filter_run', 4106, 0, 2, 8000, None, None, 1048576, None),
    ('rcfm_tuner_levels', 4098, 0, 2, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_demod_create', 3, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_pipeline_run', 4098, 4112, 2, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 2, 2, 8000, None, None, 1048578, None),
    ('rcfm_tuner_levels', 4098, 2, 2, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048584, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    # the lane: the fence on the shared filter handle, then handles of its own
    ('rcfm_audio_filter_set_fence', 4106, 1),
    ('rcfm_tuner_create', 600000, 4, [18747, 6247, -6253, -18753], [12500, 12500, 12500, 12500], REF),
    ('rcfm_tuner_set_iq_balance', 4121, 2, 0.0, 0.0, 2),
    ('rcfm_blanker_create', 600000, 4096, 4, 0, 15.848931924611133, 1, PTR, 1, REF),
    ('rcfm_blanker_run', 4123, 0, 600000, None, None, None, None),
    ('rcfm_tuner_load', 4121, None, None),
    ('rcfm_demod_create', 0, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_pipeline_run', 4121, 4126, 0, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 0, 2, 8000, None, None, 1048576, None),
    ('rcfm_tuner_levels', 4121, 0, 2, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_demod_create', 3, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_pipeline_run', 4121, 4134, 2, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 2, 2, 8000, None, None, 1048578, None),
    ('rcfm_tuner_levels', 4121, 2, 2, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048584, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    # new settings on the base reach its handle at once, the lane's with the lane's next load
    ('rcfm_tuner_retune', 4098, 0, 4, [18747, 6248, -6253, -18755], None),
    ('rcfm_tuner_set_iq_balance', 4098, 1, 0.009999999776482582, 0.019999999552965164, 0),
    ('rcfm_blanker_destroy', 4123),
    ('rcfm_blanker_create', 600000, 4096, 4, 0, 10.0, 1, PTR, 1, REF),
    ('rcfm_blanker_run', 4145, 0, 600000, None, None, None, None),
    ('rcfm_tuner_retune', 4121, 0, 4, [18747, 6248, -6253, -18755], None),
    ('rcfm_tuner_set_iq_balance', 4121, 1, 0.009999999776482582, 0.019999999552965164, 0),
    ('rcfm_tuner_load', 4121, None, None),
    ('rcfm_pipeline_run', 4121, 4126, 0, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 0, 2, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4121, 0, 2, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_pipeline_run', 4121, 4134, 2, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 2, 2, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4121, 2, 2, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048584, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    ('rcfm_blanker_run', 4145, 0, 600000, None, None, None, None),
    ('rcfm_tuner_load', 4121, None, None),
    ('rcfm_pipeline_run', 4121, 4126, 0, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 0, 2, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4121, 0, 2, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 2, 8000, None, None, None),
    ('rcfm_pipeline_run', 4121, 4134, 2, 2, None, None),
    ('rcfm_tone_bank_run', 4097, None, 2, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 2, 2, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4121, 2, 2, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048584, None, 2, 1, 39, None, None),
    ('rcfm_squelch', None, 1048584, 2, 8000, None, None, None),
    # the shard: the base's handle for its new blanker, two groups of one channel, a whole load, reset_states
    ('rcfm_tuner_shard', 4098, 1, 2),
    ('rcfm_blanker_create', 600000, 4096, 4, 0, 10.0, 1, PTR, 1, REF),
    ('rcfm_blanker_destroy', 4100),
    ('rcfm_blanker_run', 4181, 0, 600000, None, None, None, None),
    ('rcfm_tuner_load', 4098, None, None),
    ('rcfm_pipeline_run', 4098, 4103, 1, 1, None, None),
    ('rcfm_tone_bank_run', 4097, None, 1, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 1, 1, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4098, 1, 1, None, None),
    ('rcfm_squelch', None, 1048580, 1, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048580, None, 1, 1, 39, None, None),
    ('rcfm_squelch', None, 1048580, 1, 8000, None, None, None),
    ('rcfm_pipeline_run', 4098, 4112, 2, 1, None, None),
    ('rcfm_tone_bank_run', 4097, None, 1, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4106, 2, 1, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4098, 2, 1, None, None),
    ('rcfm_squelch', None, 1048584, 1, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048584, None, 1, 1, 39, None, None),
    ('rcfm_squelch', None, 1048584, 1, 8000, None, None, None),
    ('rcfm_blanker_run', 4181, 0, 600000, None, None, None, None),
    ('rcfm_tuner_shard', 4098, 0, 4),
    ('rcfm_tuner_load', 4098, None, None),
    ('rcfm_tuner_shard', 4098, 1, 2),
    ('rcfm_demod_reset_state', 4103, None),
    ('rcfm_demod_reset_state', 4112, None),
    ('rcfm_audio_filter_reset', 4106, None),
    # one class for all channels: run_all, run_all(chunk=2), run_all_packed, a kernel option, an empty shard, one more channel
    ('rcfm_tuner_create', 600000, 4, [18750, 6250, -6250, -18750], [12500, 12500, 12500, 12500], REF),
    ('rcfm_blanker_create', 600000, 4096, 4, 0, 15.848931924611133, 1, PTR, 1, REF),
    ('rcfm_blanker_run', 4207, 0, 600000, None, None, None, None),
    ('rcfm_tuner_load', 4206, None, None),
    ('rcfm_demod_create', 1, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_pipeline_run', 4206, 4210, 0, 4, None, None),
    ('rcfm_tone_bank_run', 4097, None, 4, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_create', 4, 1, 5, PTR, REF),
    ('rcfm_audio_filter_run', 4213, 0, 4, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4206, 0, 4, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 4, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_demod_create', 1, 4, 12500, 8000, 7.5e-05, 2, REF),
    ('rcfm_demod_bind_state', 4219, 4210, 0, 0, None),
    ('rcfm_pipeline_run', 4206, 4219, 0, 4, None, None),
    ('rcfm_tone_bank_run', 4097, None, 4, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4213, 0, 4, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4206, 0, 4, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 4, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_pipeline_run', 4206, 4210, 0, 4, None, None),
    ('rcfm_tone_bank_run', 4097, None, 4, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4213, 0, 4, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4206, 0, 4, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 4, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_audio_pack', None, None, 4, 8000, 1, 32767.0, None, None, None, None),
    ('rcfm_demod_create', 1, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_demod_set_option', 4236, 2, 0),
    ('rcfm_demod_bind_state', 4236, 4210, 0, 0, None),
    ('rcfm_pipeline_run', 4206, 4236, 0, 4, None, None),
    ('rcfm_tone_bank_run', 4097, None, 4, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_run', 4213, 0, 4, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4206, 0, 4, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 4, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 4, 8000, None, None, None),
    ('rcfm_tuner_shard', 4206, 0, 0),
    ('rcfm_pipeline_run', 4206, 4236, 0, 0, None, None),
    ('rcfm_tuner_shard', 4206, 0, 5),
    ('rcfm_tuner_create', 600000, 5, [25000, 12500, 0, -12500, -25000], [12500, 12500, 12500, 12500, 12500], REF),
    ('rcfm_tuner_destroy', 4206),
    ('rcfm_tuner_shard', 4249, 0, 5),
    ('rcfm_blanker_run', 4207, 0, 600000, None, None, None, None),
    ('rcfm_tuner_load', 4249, None, None),
    ('rcfm_demod_create', 1, 5, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_demod_set_option', 4254, 2, 0),
    ('rcfm_pipeline_run', 4249, 4254, 0, 5, None, None),
    ('rcfm_tone_bank_run', 4097, None, 5, 8000, 1, 0, None, None, None),
    ('rcfm_audio_filter_create', 5, 1, 5, PTR, REF),
    ('rcfm_audio_filter_get_state', 4213, PTR, None),
    ('rcfm_audio_filter_set_state', 4258, PTR, None),
    ('rcfm_audio_filter_destroy', 4213),
    ('rcfm_audio_filter_run', 4258, 0, 5, 8000, None, None, None, None),
    ('rcfm_tuner_levels', 4249, 0, 5, None, None),
    ('rcfm_squelch', None, 1048576, 5, 8000, None, None, None),
    ('rcfm_tone_score', None, None, 1048576, None, 5, 1, 39, None, None),
    ('rcfm_squelch', None, 1048576, 5, 8000, None, None, None),
    # the carried stages on a third tuner: the floor's pass behind the load, then mixer and bus dynamics (made before the first
    # launch), demodulator, filter, gate over the floor's thresholds, mixer, bus dynamics
    ('rcfm_tuner_create', 600000, 4, [18750, 6250, -6250, -18750], [12500, 12500, 12500, 12500], REF),
    ('rcfm_tuner_load', 4267, None, None),
    ('rcfm_tuner_power_spectrum', 4267, -300000, 600000, 600, None, None, None),
    ('rcfm_floor_create', 600, 40, 8, 250, 0.09516258537769318, 0.6321205496788025, REF),
    ('rcfm_floor_run', 4270, None, 1.0, None, None, None),
    ('rcfm_floor_thresholds', None, 600, None, None, 12, None, None),
    ('rcfm_mix_create', 2, PTR, PTR, PTR, 2, REF),
    ('rcfm_busdyn_create', 2, 2, 64, 8000, 0.8912509083747864, 0.0314934179186821, PTR, PTR, PTR, PTR, REF),
    ('rcfm_demod_create', 1, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_pipeline_run', 4267, 4275, 0, 4, None, None),
    ('rcfm_audio_filter_create', 4, 1, 5, PTR, REF),
    ('rcfm_audio_filter_run', 4277, 0, 4, 8000, None, None, None, None),
    ('rcfm_gate_create', 4, 12, 1, PTR, 40, REF),
    ('rcfm_tuner_frame_levels', 4267, 0, 4, 50, None, 400000, None, None),
    ('rcfm_gate_run', 4279, 0, 4, 50, None, 1048592, 1048608, None, None, None),
    ('rcfm_gate_apply', 4279, None, 4, 50, 8000, 1, None, None),
    ('rcfm_mix_run', 4273, 0, 4, 8000, 1, None, None, None, None, None, None),
    ('rcfm_busdyn_run', 4274, 8000, None, None, None, None, None),
    # _arm_state_fence(): the batched demodulator, then audio filter, gate, floor, bus dynamics (the mixer has no state)
    ('rcfm_demod_set_option', 4275, 5, 1),
    ('rcfm_audio_filter_set_fence', 4277, 1),
    ('rcfm_gate_set_fence', 4279, 1),
    ('rcfm_floor_set_fence', 4270, 1),
    ('rcfm_busdyn_set_fence', 4274, 1),
    # the lane: handles of its own for tuner and demodulator (bound to the base's state), every carried handle shared
    ('rcfm_tuner_create', 600000, 4, [18750, 6250, -6250, -18750], [12500, 12500, 12500, 12500], REF),
    ('rcfm_tuner_load', 4290, None, None),
    ('rcfm_tuner_power_spectrum', 4290, -300000, 600000, 600, None, None, None),
    ('rcfm_floor_run', 4270, None, 1.0, None, None, None),
    ('rcfm_floor_thresholds', None, 600, None, None, 12, None, None),
    ('rcfm_demod_create', 1, 4, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_demod_bind_state', 4295, 4275, 0, 0, None),
    ('rcfm_demod_set_option', 4295, 5, 1),
    ('rcfm_pipeline_run', 4290, 4295, 0, 4, None, None),
    ('rcfm_audio_filter_run', 4277, 0, 4, 8000, None, None, None, None),
    ('rcfm_tuner_frame_levels', 4290, 0, 4, 50, None, 400000, None, None),
    ('rcfm_gate_run', 4279, 0, 4, 50, None, 1048592, 1048608, None, None, None),
    ('rcfm_gate_apply', 4279, None, 4, 50, 8000, 1, None, None),
    ('rcfm_mix_run', 4273, 0, 4, 8000, 1, None, None, None, None, None, None),
    ('rcfm_busdyn_run', 4274, 8000, None, None, None, None, None),
    # new bus dynamics on the base: the old handle goes at once, the lane makes the new one and it is fenced when stored
    ('rcfm_busdyn_destroy', 4274),
    ('rcfm_tuner_load', 4290, None, None),
    ('rcfm_tuner_power_spectrum', 4290, -300000, 600000, 600, None, None, None),
    ('rcfm_floor_run', 4270, None, 1.0, None, None, None),
    ('rcfm_floor_thresholds', None, 600, None, None, 12, None, None),
    ('rcfm_busdyn_create', 2, 2, 16, 8000, 0.8912509083747864, 0.007968084886670113, None, None, None, None, REF),
    ('rcfm_busdyn_set_fence', 4310, 1),
    ('rcfm_pipeline_run', 4290, 4295, 0, 4, None, None),
    ('rcfm_audio_filter_run', 4277, 0, 4, 8000, None, None, None, None),
    ('rcfm_tuner_frame_levels', 4290, 0, 4, 50, None, 400000, None, None),
    ('rcfm_gate_run', 4279, 0, 4, 50, None, 1048592, 1048608, None, None, None),
    ('rcfm_gate_apply', 4279, None, 4, 50, 8000, 1, None, None),
    ('rcfm_mix_run', 4273, 0, 4, 8000, 1, None, None, None, None, None, None),
    ('rcfm_busdyn_run', 4310, 8000, None, None, None, None, None),
    # one more channel: a new mixer handle; the filter's and the gate's states move into longer handles, fenced when stored
    ('rcfm_tuner_create', 600000, 5, [25000, 12500, 0, -12500, -25000], [12500, 12500, 12500, 12500, 12500], REF),
    ('rcfm_tuner_destroy', 4267),
    ('rcfm_tuner_load', 4319, None, None),
    ('rcfm_tuner_power_spectrum', 4319, -300000, 600000, 600, None, None, None),
    ('rcfm_floor_run', 4270, None, 1.0, None, None, None),
    ('rcfm_floor_thresholds', None, 600, None, None, 15, None, None),
    ('rcfm_mix_destroy', 4273),
    ('rcfm_mix_create', 2, PTR, PTR, PTR, 2, REF),
    ('rcfm_demod_create', 1, 5, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_demod_set_option', 4327, 5, 1),
    ('rcfm_pipeline_run', 4319, 4327, 0, 5, None, None),
    ('rcfm_audio_filter_create', 5, 1, 5, PTR, REF),
    ('rcfm_audio_filter_get_state', 4277, PTR, None),
    ('rcfm_audio_filter_set_state', 4330, PTR, None),
    ('rcfm_audio_filter_set_fence', 4330, 1),
    ('rcfm_audio_filter_destroy', 4277),
    ('rcfm_audio_filter_run', 4330, 0, 5, 8000, None, None, None, None),
    ('rcfm_gate_create', 5, 12, 1, PTR, 40, REF),
    ('rcfm_gate_get_state', 4279, PTR, None),
    ('rcfm_gate_set_state', 4336, PTR, None),
    ('rcfm_gate_set_fence', 4336, 1),
    ('rcfm_gate_destroy', 4279),
    ('rcfm_tuner_frame_levels', 4319, 0, 5, 50, None, 500000, None, None),
    ('rcfm_gate_run', 4336, 0, 5, 50, None, 1048596, 1048616, None, None, None),
    ('rcfm_gate_apply', 4336, None, 5, 50, 8000, 1, None, None),
    ('rcfm_mix_run', 4326, 0, 5, 8000, 1, None, None, None, None, None, None),
    ('rcfm_busdyn_run', 4310, 8000, None, None, None, None, None),
    ('rcfm_tuner_create', 600000, 5, [25000, 12500, 0, -12500, -25000], [12500, 12500, 12500, 12500, 12500], REF),
    ('rcfm_tuner_destroy', 4290),
    ('rcfm_tuner_load', 4346, None, None),
    ('rcfm_tuner_power_spectrum', 4346, -300000, 600000, 600, None, None, None),
    ('rcfm_floor_run', 4270, None, 1.0, None, None, None),
    ('rcfm_floor_thresholds', None, 600, None, None, 15, None, None),
    ('rcfm_demod_create', 1, 5, 12500, 8000, 7.5e-05, 0, REF),
    ('rcfm_demod_bind_state', 4352, 4327, 0, 0, None),
    ('rcfm_demod_set_option', 4352, 5, 1),
    ('rcfm_pipeline_run', 4346, 4352, 0, 5, None, None),
    ('rcfm_audio_filter_run', 4330, 0, 5, 8000, None, None, None, None),
    ('rcfm_tuner_frame_levels', 4346, 0, 5, 50, None, 500000, None, None),
    ('rcfm_gate_run', 4336, 0, 5, 50, None, 1048596, 1048616, None, None, None),
    ('rcfm_gate_apply', 4336, None, 5, 50, 8000, 1, None, None),
    ('rcfm_mix_run', 4326, 0, 5, 8000, 1, None, None, None, None, None, None),
    ('rcfm_busdyn_run', 4310, 8000, None, None, None, None, None),
    # reset_states(): the batched demodulators, then audio filter, gate, floor, bus dynamics
    ('rcfm_demod_reset_state', 4275, None),
    ('rcfm_demod_reset_state', 4327, None),
    ('rcfm_audio_filter_reset', 4330, None),
    ('rcfm_gate_reset', 4336, None),
    ('rcfm_floor_reset', 4270, None),
    ('rcfm_busdyn_reset', 4310, None),
    # reset(): every carried cache goes, in the order they are held: filter, gate, floor, mixer, bus dynamics
    ('rcfm_audio_filter_destroy', 4330),
    ('rcfm_gate_destroy', 4336),
    ('rcfm_floor_destroy', 4270),
    ('rcfm_mix_destroy', 4326),
    ('rcfm_busdyn_destroy', 4310),
    # every stage off: what the settings held goes, then a load and a run and nothing else
    ('rcfm_audio_filter_destroy', 4258),
    ('rcfm_tuner_set_iq_balance', 4249, 0, 0.0, 0.0, 0),
    ('rcfm_blanker_destroy', 4207),
    ('rcfm_tuner_load', 4249, None, None),
    ('rcfm_pipeline_run', 4249, 4254, 0, 5, None, None),
]
