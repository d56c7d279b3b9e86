"""The audio buses' entry points (include/rcfm.h: rcfm_mix_create / _run / _destroy): declared, exported, bound, and refusing
every bad argument before any device call -- none of this needs a device -- and Tuner.set_mix / Tuner.mix /
run_all_packed(buses=True) / Lanes on the host, against a library that counts its calls.  What needs a handle needs a
device: tests/test_hip_mix.py."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_mix_create", "rcfm_mix_run", "rcfm_mix_destroy")
ERR_ARG, ERR_INDEX = -4, -2
_vp, _i = ctypes.c_void_p, ctypes.c_int
_ip, _fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    lib.rcfm_mix_create.argtypes = [_i, _ip, _ip, _fp, _i, ctypes.POINTER(_vp)]
    lib.rcfm_mix_run.argtypes = [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.rcfm_mix_destroy.argtypes = [_vp]
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert re.search(r"typedef\s+struct\s+rcfm_mix_s\s*\*\s*rcfm_mix_t\s*;", header)
    assert [len(hip.SIGNATURES[n]) for n in NEW] == [6, 11, 1]
    # the limits the Python layer uses are the kernel's own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "mix.h")).read()
    assert re.search(r"kMixMaxBuses\s*=\s*%d\b" % hip.RCFM_MIX_MAX_BUSES, kernel)
    assert re.search(r"kMixMaxBusRoutes\s*=\s*%d\b" % hip.RCFM_MIX_MAX_BUS_ROUTES, kernel)
    assert re.search(r"kMixMaxRoutes\s*=\s*1\s*<<\s*20\b", kernel) and hip.RCFM_MIX_MAX_ROUTES == 1 << 20
    assert re.search(r"kMixSegment\s*=\s*%d\b" % hip.RCFM_MIX_SEGMENT, kernel) and hip.RCFM_MIX_SEGMENT == 16
    assert lib.rcfm_version() == 102
    # no profile stage was added: the list still ends with the squelch's
    lib.rcfm_profile_stage_name.restype = ctypes.c_char_p
    lib.rcfm_profile_stage_name.argtypes = [_i]
    assert lib.rcfm_profile_stage_name(lib.rcfm_profile_stage_count() - 1) == b"squelch"


def _refused(lib, status, word, code=ERR_ARG):
    assert status == code, status
    assert word in lib.rcfm_last_error(), (word, lib.rcfm_last_error())


def _tables(start, chan, gain):
    s = np.ascontiguousarray(start, dtype=np.int32)
    c = np.ascontiguousarray(chan, dtype=np.int32)
    g = np.ascontiguousarray(gain, dtype=np.float32)
    return (s, c, g), (s.ctypes.data_as(_ip), c.ctypes.data_as(_ip), g.ctypes.data_as(_fp))


def test_create_refuses_before_any_device_call(lib):
    out = _vp()
    create = lib.rcfm_mix_create
    keep, (s, c, g) = _tables([0, 2, 3], [4, 7, 4], [[1.0, 0.5]] * 3)
    _refused(lib, create(2, None, c, g, 2, ctypes.byref(out)), b"NULL")
    _refused(lib, create(2, s, None, g, 2, ctypes.byref(out)), b"NULL")
    _refused(lib, create(2, s, c, None, 2, ctypes.byref(out)), b"NULL")
    _refused(lib, create(2, s, c, g, 2, None), b"NULL")
    for M in (0, -1, 1025):
        _refused(lib, create(M, s, c, g, 2, ctypes.byref(out)), b"M outside")
    for ch_out in (0, 3, -1):
        _refused(lib, create(2, s, c, g, ch_out, ctypes.byref(out)), b"ch_out outside")

    def tables(start, chan=None, gain=None):
        R = max(int(max(start)), 1)
        chan = np.arange(R) % 65535 if chan is None else chan
        gain = np.ones((R, 2)) if gain is None else gain
        return _tables(start, chan, gain)
    keep2, (s2, c2, g2) = tables([1, 2, 3])
    _refused(lib, create(2, s2, c2, g2, 2, ctypes.byref(out)), b"bus_start[0]")
    keep3, (s3, c3, g3) = tables([0, 3, 2])
    _refused(lib, create(2, s3, c3, g3, 2, ctypes.byref(out)), b"not monotone")
    keep4, (s4, c4, g4) = tables([0, 65536])
    _refused(lib, create(1, s4, c4, g4, 2, ctypes.byref(out)), b"more than 65535 routes")
    keep5, (s5, c5, g5) = tables([65535 * m for m in range(18)])                # 17 x 65 535 > 2^20
    _refused(lib, create(17, s5, c5, g5, 2, ctypes.byref(out)), b"more than 2^20 routes")
    keep6, (s6, c6, g6) = tables([0, 2, 3], chan=[4, -1, 4])
    _refused(lib, create(2, s6, c6, g6, 2, ctypes.byref(out)), b"negative channel")
    keep7, (s7, c7, g7) = tables([0, 3, 3], chan=[4, 7, 4])
    _refused(lib, create(2, s7, c7, g7, 2, ctypes.byref(out)), b"twice in one bus")
    for bad in (np.nan, np.inf, -np.inf):
        for leg in (0, 1):
            gain = np.ones((3, 2))
            gain[1, leg] = bad
            keep8, (s8, c8, g8) = tables([0, 2, 3], chan=[4, 7, 4], gain=gain)
            _refused(lib, create(2, s8, c8, g8, 2, ctypes.byref(out)), b"not finite")
    assert not out.value
    assert lib.rcfm_mix_destroy(None) == 0


def test_run_refuses_before_any_device_call(lib):
    p, p2, odd = _vp(0x100000), _vp(0x900000), _vp(0x100002)          # never dereferenced
    h = _vp(0x200000)                              # stands for a handle: every call below is refused before it is read
    run = lib.rcfm_mix_run
    _refused(lib, run(None, 0, 4, 100, 1, p, None, p2, None, None, None), b"NULL")
    _refused(lib, run(h, 0, 4, 100, 1, None, None, p2, None, None, None), b"NULL")
    _refused(lib, run(h, 0, 4, 100, 1, p, None, None, None, None, None), b"NULL")
    for ch_in in (0, 3, -2):
        _refused(lib, run(h, 0, 4, 100, ch_in, p, None, p2, None, None, None), b"ch_in outside")
    for count in (0, -1):
        _refused(lib, run(h, 0, count, 100, 1, p, None, p2, None, None, None), b"count below 1")
    for A in (0, -5):
        _refused(lib, run(h, 0, 4, A, 1, p, None, p2, None, None, None), b"A below 1")
    _refused(lib, run(h, 0, 4, 100, 1, odd, None, p2, None, None, None), b"misaligned")
    _refused(lib, run(h, 0, 4, 100, 1, p, None, odd, None, None, None), b"misaligned")
    _refused(lib, run(h, 0, 4, 100, 1, p, None, p2, odd, None, None), b"misaligned")


def test_set_mix_on_the_host(monkeypatch):
    """Tuner.set_mix: off by default and then no rcfm_mix_* call; set, rcfm_mix_run follows the squelch / gate / tone squelch
    of its group on their mask; one handle per group, reused by the next run; refused across groups, under shard, with a
    window attached and for a channel the tuner does not have; lanes share setting and handles; reset() drops them;
    run_all_packed(buses=True) hands `out` and `bus_open` to rcfm_audio_pack."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    from radiocore.tools.gate import FrameGate

    ids = iter(range(1, 1 << 30))

    class _Tensor(_FakeTensor):
        dtype = "f32"

        def __init__(self, shape):
            super().__init__(shape)
            self.addr = 0x100000 * next(ids)

        def data_ptr(self):
            return self.addr

        def is_contiguous(self):
            return True

        def numel(self):
            return int(np.prod(self.shape))

    class _Torch(_FakeTorch):
        Tensor = _Tensor
        uint8 = "u8"
        int32 = "i32"
        int16 = "i16"

    fake = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: fake)
    monkeypatch.setattr(hip, "torch", lambda: _Torch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _Tensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: t.data_ptr())
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_host", lambda x: x)
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _Tensor(getattr(x, "shape", (len(x),))))
    import radiocore as rc
    B, A, C, N = 12500, 8000, 6, 600000
    MIX = ("rcfm_mix_create", "rcfm_mix_run", "rcfm_mix_destroy")

    def tuner(channels=C, wide=0):
        t = rc.Tuner()
        for i in range(channels):
            t.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
        for i in range(wide):                       # a second launch group: another bandwidth
            t.add_channel(446.0e6 + float(B) * channels + 25000.0 * i + 6250.0, 25000, rc.FM(25000, A))
        t.request_bandwidth(float(N))
        return t

    def mix_calls(since=0):
        return [(n, a) for n, a in fake.calls[since:] if n in MIX]
    t = tuner()
    x = np.zeros(N, np.complex64)
    # off by default: nothing of the mixer's
    assert t._mix is None
    t.set_squelch(1e-3)
    t.load(x)
    t.run_all()
    assert not mix_calls()
    for read in (t.mix, t.mix_active):
        with pytest.raises(RuntimeError):
            read()
    with pytest.raises(ValueError):
        t.run_all_packed(rc.PCM("int16"), buses=True)
    # refusals: the setting in force stays
    for bad in ("mixer", 3, rc.Bus.of([0])):
        with pytest.raises(ValueError):
            t.set_mix(bad)
    with pytest.raises(ValueError):
        t.set_mix(rc.Mixer([rc.Bus.of([0, C])]))                        # channel 6 of a tuner with six
    assert t._mix is None and not mix_calls()
    # set: one create, and the run follows the group's squelch on its mask
    tower, rest = rc.Bus.of([1, 3], pan=[-0.5, 0.5], name="tower"), rc.Bus.of([0, 2, 4, 5], gain_db=-6.0, name="rest")
    mixer = rc.Mixer([tower, rest])
    t.set_mix(mixer)
    before = len(fake.calls)
    t.run_all()
    names = [n for n, _ in fake.calls[before:]]
    assert names.count("rcfm_mix_create") == 1 and names.count("rcfm_mix_run") == 1
    assert names.index("rcfm_pipeline_run") < names.index("rcfm_squelch") < names.index("rcfm_mix_run") == len(names) - 1
    create = [a for n, a in mix_calls(before) if n == "rcfm_mix_create"][0]
    assert create[0] == 2 and create[4] == 2
    run = [a for n, a in mix_calls(before) if n == "rcfm_mix_run"][0]
    squelch = [a for n, a in fake.calls[before:] if n == "rcfm_squelch"][0]
    pipeline = [a for n, a in fake.calls[before:] if n == "rcfm_pipeline_run"][0]
    assert run[1:5] == (0, C, A, 1)
    assert run[5] == pipeline[4] == squelch[4] and run[6] == squelch[5]             # the group's audio, the squelch's mask
    out, active, bus_open = t._last.mix[1][0]
    assert out.shape == (2, A, 2) and active.shape == (2,) and bus_open.shape == (2,)
    assert run[7:10] == (out.data_ptr(), active.data_ptr(), bus_open.data_ptr())
    assert t.mix() is out
    # the next run uses the same handle
    t.load(x)
    t.run_all()
    assert fake.count("rcfm_mix_create") == 1 and fake.count("rcfm_mix_run") == 2
    assert [a for n, a in mix_calls() if n == "rcfm_mix_run"][1][0] == run[0]
    # without a squelch the mask is NULL: every channel is open
    t.set_squelch(None)
    t.run_all()
    assert [a for n, a in mix_calls() if n == "rcfm_mix_run"][-1][6] is None
    # behind the frame gate's apply, and behind the tone squelch's rcfm_squelch, on the final mask
    t.set_gate(FrameGate(frames=50), open=1e-3)
    t.set_tones(rc.ToneBank([67.0, 71.9], frame=800), want=0, ratio=0.5)
    before = len(fake.calls)
    t.run_all()
    names = [n for n, _ in fake.calls[before:]]
    assert names.index("rcfm_gate_apply") < names.index("rcfm_tone_score") < names.index("rcfm_squelch") < names.index("rcfm_mix_run")
    assert names[-1] == "rcfm_mix_run"
    assert [a for n, a in fake.calls[before:] if n == "rcfm_mix_run"][0][6] == [a for n, a in fake.calls[before:] if n == "rcfm_squelch"][0][5]
    t.set_tones(None)
    t.set_gate(None)
    # run_all_packed(buses=True): the pack reads the bus rows and bus_open; M rows of A ch_out
    t.set_squelch(1e-3)
    drain = rc.Drain(2, (A, 2), "int16", depth=2)
    before = len(fake.calls)
    assert t.run_all_packed(rc.PCM("int16"), drain=drain, buses=True) is None
    pack = [a for n, a in fake.calls[before:] if n == "rcfm_audio_pack"][0]
    out, active, bus_open = t._last.mix[1][0]
    assert pack[0] == out.data_ptr() and pack[1] == bus_open.data_ptr() and pack[2] == 2 and pack[3] == 2 * A
    assert [n for n, _ in fake.calls[before:]][-3:] == ["rcfm_mix_run", "rcfm_audio_pack", "rcfm_drain_submit"]
    # the drain's geometry is checked against M rows of [A, ch_out], before anything is launched
    before = len(fake.calls)
    for bad in (rc.Drain(1, (A, 2), "int16"), rc.Drain(2, (A, 1), "int16"), rc.Drain(C, (A, 1), "int16")):
        with pytest.raises(ValueError):
            t.run_all_packed(rc.PCM("int16"), drain=bad, buses=True)
    assert not [n for n, _ in fake.calls[before:] if n in ("rcfm_pipeline_run", "rcfm_mix_run", "rcfm_audio_pack")]
    channel_drain = rc.Drain(C, (A, 1), "int16")
    t.run_all_packed(rc.PCM("int16"), drain=channel_drain)                             # without buses: the channel rows, as ever
    pack = [a for n, a in fake.calls[before:] if n == "rcfm_audio_pack"][0]
    assert pack[2] == C and pack[3] == A and pack[0] == [a for n, a in fake.calls[before:] if n == "rcfm_pipeline_run"][0][4]
    # a growing channel list: routes name indices; a new handle for the new list, the old one goes
    t.add_channel(446.0e6 + float(B) * C, B, rc.FM(B, A))
    t.request_bandwidth(float(N))
    t.load(x)
    t.run_all()
    assert fake.count("rcfm_mix_create") == 2 and len(t._mix_handles) == 1
    assert [a for n, a in mix_calls() if n == "rcfm_mix_run"][-1][1:3] == (0, C + 1)
    # lanes share the setting and the handles: no further create
    lane = t._lane_clone()
    assert lane._mix is mixer and lane._mix_handles is t._mix_handles
    lane.load(x)
    lane.run_all()
    assert fake.count("rcfm_mix_create") == 2
    other = rc.Mixer([tower])
    t.set_mix(other)
    assert not t._mix_handles
    lane._sync_lane(t)
    assert lane._mix is other
    lane.run_all()
    t.run_all()
    assert fake.count("rcfm_mix_create") == 3                                          # made by the lane, used by both
    # off again: nothing more of the mixer's, and the handles are gone
    t.set_mix(None)
    assert not t._mix_handles
    before = len(fake.calls)
    t.load(x)
    t.run_all()
    assert not [n for n, _ in mix_calls(before) if n != "rcfm_mix_destroy"]
    with pytest.raises(RuntimeError):
        t.mix()
    # reset() drops the handles; a route to a channel that is gone is refused at the next run, before anything is launched
    t.set_mix(mixer)
    t.run_all()
    assert t._mix_handles
    with pytest.raises(ValueError):
        t.reset()
    assert not t._mix_handles
    for i in range(3):
        t.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
    t.request_bandwidth(float(N))
    t.load(x)
    before = len(fake.calls)
    with pytest.raises(ValueError):
        t.run_all()
    assert not [n for n, _ in fake.calls[before:] if n in ("rcfm_pipeline_run", "rcfm_mix_run")]
    # run_each: one handle per group; a bus across two groups is refused before anything is launched
    e = tuner(channels=4, wide=2)
    e.set_mix(rc.Mixer([rc.Bus.of([0, 1, 3]), rc.Bus.of([5, 4]), rc.Bus([])]))
    e.load(x)
    before = len(fake.calls)
    e.run_each()
    runs = [a for n, a in mix_calls(before) if n == "rcfm_mix_run"]
    assert [n for n, _ in mix_calls(before)].count("rcfm_mix_create") == 2
    assert [r[1:3] for r in runs] == [(0, 4), (4, 2)] and runs[0][0] != runs[1][0]
    assert e._last.mix[0] == [0, 1, 0] and len(e.mix()) == 3
    e.run_each()
    assert [n for n, _ in mix_calls(before)].count("rcfm_mix_create") == 2              # reused
    e.set_mix(rc.Mixer([rc.Bus.of([3, 4])]))
    before = len(fake.calls)
    with pytest.raises(ValueError, match="launch groups"):
        e.run_each()
    assert not [n for n, _ in fake.calls[before:] if n in ("rcfm_pipeline_run", "rcfm_mix_run")]
    # under shard and with a window attached: refused, as set_floor is
    sharded = tuner()
    sharded.shard(0, 2)
    with pytest.raises(ValueError):
        sharded.set_mix(mixer)
    assert sharded._mix is None
    late = tuner()
    late.set_mix(mixer)
    late.shard(0, 3)
    late.load(x)
    before = len(fake.calls)
    with pytest.raises(RuntimeError):
        late.run_all()
    assert not [n for n, _ in fake.calls[before:] if n in ("rcfm_pipeline_run", "rcfm_mix_run")]
    attached = tuner()
    attached._slot = object()
    with pytest.raises(ValueError):
        attached.set_mix(mixer)
