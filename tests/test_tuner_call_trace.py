"""CPU: the whole sequence of ABI calls the Tuner makes with every optional stage on at once -- squelch, tone bank and tone
squelch, audio filter, IQ balance, blanker, retune, shard, lanes, chunked and packed runs, kernel options -- pinned call by
call against a literal list.  The library is the counting stand-in of tests/test_am.py; no device is used.  The list is
what the library sees: a change of the Tuner that leaves behaviour alone leaves this test alone."""

import ctypes

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
    return off, (t, lane, u, bank)


def test_the_call_sequence_of_every_stage_at_once(fake):
    off, alive = _scenario(fake)         # (the trace ends before the tuners go: what is destroyed in between is part of it)
    assert _names(fake, off) == ["rcfm_tuner_load", "rcfm_pipeline_run"]
    got = _trace(fake)
    for i, (g, w) in enumerate(zip(got, EXPECTED)):
        assert g == w, (i, g, w)
    assert len(got) == len(EXPECTED)


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
    # every stage off: what the settings held goes, then a load and a run and nothing else
    ('rcfm_audio_filter_destroy', 4258),
    ('rcfm_tuner_set_iq_balance', 4249, 0, 0.0, 0.0, 0),
    ('rcfm_blanker_destroy', 4207),
    ('rcfm_tuner_load', 4249, None, None),
    ('rcfm_pipeline_run', 4249, 4254, 0, 5, None, None),
]
