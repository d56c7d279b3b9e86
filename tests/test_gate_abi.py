"""The frame gate's entry points (include/rcfm.h: rcfm_frame_power, rcfm_tuner_frame_levels, rcfm_gate_create / _run / _apply /
_reset / _get_state / _set_state / _set_fence / _destroy): declared, exported, bound, and refusing every bad argument
before any device call -- none of this needs a device.  RCFM_ERR_INDEX and the ramp-against-frame check need a handle, and a
handle needs a device: tests/test_hip_gate.py."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_frame_power", "rcfm_tuner_frame_levels", "rcfm_gate_create", "rcfm_gate_run", "rcfm_gate_apply", "rcfm_gate_reset",
       "rcfm_gate_get_state", "rcfm_gate_set_state", "rcfm_gate_set_fence", "rcfm_gate_destroy")
ERR_ARG = -4
_vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
_fp, _ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    lib.rcfm_frame_power.argtypes = [_vp, _i, _i64, _i, _i, _vp, _vp]
    lib.rcfm_tuner_frame_levels.argtypes = [_vp, _i, _i, _i, _vp, _sz, _vp, _vp]
    lib.rcfm_gate_create.argtypes = [_i, _i, _i, _fp, _i, ctypes.POINTER(_vp)]
    lib.rcfm_gate_run.argtypes = [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.rcfm_gate_apply.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp]
    lib.rcfm_gate_reset.argtypes = [_vp, _vp]
    lib.rcfm_gate_get_state.argtypes = [_vp, _ip, _vp]
    lib.rcfm_gate_set_state.argtypes = [_vp, _ip, _vp]
    lib.rcfm_gate_set_fence.argtypes = [_vp, _i]
    lib.rcfm_gate_destroy.argtypes = [_vp]
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert re.search(r"typedef\s+struct\s+rcfm_gate_s\s*\*\s*rcfm_gate_t\s*;", header)
    assert [len(hip.SIGNATURES[n]) for n in NEW] == [7, 8, 6, 10, 8, 2, 3, 3, 2, 1]
    # the limits the Python layer uses are the kernel's own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "gate.h")).read()
    for name, value in (("kGateWaveFloats", hip.RCFM_GATE_WAVE_FLOATS), ("kGateSegFloats", hip.RCFM_GATE_SEG_FLOATS),
                        ("kGateMaxFrames", hip.RCFM_GATE_MAX_FRAMES)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), kernel), name
    assert re.search(r"kGateMaxRamp\s*=\s*1\s*<<\s*20\b", kernel) and hip.RCFM_GATE_MAX_RAMP == 1 << 20
    assert lib.rcfm_version() == 102
    # no profile stage was added: the list still ends with the squelch's
    lib.rcfm_profile_stage_name.restype = ctypes.c_char_p
    lib.rcfm_profile_stage_name.argtypes = [_i]
    assert lib.rcfm_profile_stage_name(lib.rcfm_profile_stage_count() - 1) == b"squelch"


def _refused(lib, status, word, code=ERR_ARG):
    assert status == code, status
    assert word in lib.rcfm_last_error(), (word, lib.rcfm_last_error())


def test_frame_power_refuses_before_any_device_call(lib):
    p, odd4, odd2 = _vp(0x100000), _vp(0x100004), _vp(0x100002)          # never dereferenced
    fp = lib.rcfm_frame_power
    _refused(lib, fp(None, 1, 100, 0, 10, p, None), b"NULL")
    _refused(lib, fp(p, 1, 100, 0, 10, None, None), b"NULL")
    _refused(lib, fp(p, -1, 100, 0, 10, p, None), b"negative row count")
    for L, n in ((0, 100), (-5, 100), (101, 100), (1, 0), (2 ** 31 - 1, 10)):
        _refused(lib, fp(p, 1, n, 1, L, p, None), b"outside 1 .. n")
    _refused(lib, fp(p, 1, 2 ** 32, 0, 2 ** 30 + 1, p, None), b"above 2^30")
    _refused(lib, fp(odd2, 1, 100, 0, 10, p, None), b"misaligned")
    _refused(lib, fp(odd4, 1, 100, 1, 10, p, None), b"misaligned")          # complex rows start on 8-byte boundaries
    _refused(lib, fp(p, 1, 100, 0, 10, odd2, None), b"misaligned")
    _refused(lib, fp(p, 2 ** 31 - 1, 100, 0, 1, p, None), b"too many frames")
    assert fp(p, 0, 100, 1, 10, p, None) == 0                                # no rows: nothing is launched


def test_frame_levels_refuses_before_any_device_call(lib):
    p, odd = _vp(0x100000), _vp(0x100004)
    h = _vp(0x200000)                              # stands for a handle: every call below is refused before it is read
    fl = lib.rcfm_tuner_frame_levels
    _refused(lib, fl(None, 0, 1, 10, p, 1 << 20, p, None), b"NULL")
    _refused(lib, fl(h, 0, 1, 10, None, 1 << 20, p, None), b"NULL")
    _refused(lib, fl(h, 0, 1, 10, p, 1 << 20, None, None), b"NULL")
    for F in (0, -1):
        _refused(lib, fl(h, 0, 1, F, p, 1 << 20, p, None), b"F must be at least 1")
    _refused(lib, fl(h, 0, 1, 10, odd, 1 << 20, p, None), b"misaligned")
    _refused(lib, fl(h, 0, 1, 10, p, 1 << 20, _vp(0x100002), None), b"misaligned")


def test_gate_create_refuses_before_any_device_call(lib):
    out = _vp()
    create = lib.rcfm_gate_create
    ramp = (ctypes.c_float * 4)(0.1, 0.35, 0.65, 0.9)
    _refused(lib, create(1, 0, 0, ramp, 4, None), b"NULL")
    for C in (0, -1):
        _refused(lib, create(C, 0, 0, ramp, 4, ctypes.byref(out)), b"C must be at least 1")
    for hang, lead in ((-1, 0), (0, -1)):
        _refused(lib, create(1, hang, lead, ramp, 4, ctypes.byref(out)), b"hang and lead")
    for R in (-1, (1 << 20) + 1):
        _refused(lib, create(1, 0, 0, ramp, R, ctypes.byref(out)), b"ramp length")
    _refused(lib, create(1, 0, 0, None, 4, ctypes.byref(out)), b"NULL")
    for bad in (float("nan"), float("inf")):
        _refused(lib, create(1, 0, 0, (ctypes.c_float * 4)(0.1, bad, 0.65, 0.9), 4, ctypes.byref(out)), b"not finite")
    assert not out.value


def test_the_other_entry_points_refuse_before_any_device_call(lib):
    p, odd = _vp(0x100000), _vp(0x100002)          # never dereferenced
    h = _vp(0x200000)                              # stands for a handle: every call below is refused before it is read
    run, apply = lib.rcfm_gate_run, lib.rcfm_gate_apply
    _refused(lib, run(None, 0, 1, 10, p, p, p, p, p, None), b"NULL")
    for k in range(4):                             # power, open_thr, close_thr, frame_mask; open_any may be NULL
        args = [p, p, p, p]
        args[k] = None
        _refused(lib, run(h, 0, 1, 10, *args, None, None), b"NULL")
    _refused(lib, run(h, 0, -1, 10, p, p, p, p, None, None), b"negative channel count")
    for F in (0, -1, 65536):
        _refused(lib, run(h, 0, 1, F, p, p, p, p, None, None), b"F outside")
    for k in range(3):
        args = [p, p, p]
        args[k] = odd
        _refused(lib, run(h, 0, 1, 10, *args, p, None, None), b"misaligned")
    _refused(lib, apply(None, p, 1, 10, 800, 1, p, None), b"NULL")
    _refused(lib, apply(h, None, 1, 10, 800, 1, p, None), b"NULL")
    _refused(lib, apply(h, p, 1, 10, 800, 1, None, None), b"NULL")
    _refused(lib, apply(h, p, -1, 10, 800, 1, p, None), b"negative channel count")
    for F in (0, -1, 65536):
        _refused(lib, apply(h, p, 1, F, 800, 1, p, None), b"F outside")
    for A, F in ((0, 10), (-800, 10), (801, 10), (5, 10)):
        _refused(lib, apply(h, p, 1, F, A, 1, p, None), b"does not divide")
    for ch in (0, 3, -1):
        _refused(lib, apply(h, p, 1, 10, 800, ch, p, None), b"ch is 1 or 2")
    _refused(lib, apply(h, p, 1, 10, 800, 1, odd, None), b"misaligned")
    state = (ctypes.c_int32 * 2)()
    _refused(lib, lib.rcfm_gate_reset(None, None), b"NULL")
    _refused(lib, lib.rcfm_gate_get_state(None, state, None), b"NULL")
    _refused(lib, lib.rcfm_gate_get_state(h, None, None), b"NULL")
    _refused(lib, lib.rcfm_gate_set_state(None, state, None), b"NULL")
    _refused(lib, lib.rcfm_gate_set_state(h, None, None), b"NULL")
    _refused(lib, lib.rcfm_gate_set_fence(None, 1), b"NULL")
    assert lib.rcfm_gate_destroy(None) == 0


def test_set_gate_on_the_host(monkeypatch):
    """Tuner.set_gate: off by default, refusals with the setting in force kept, for channels added later in the next run
    before anything is launched; the run queues frame levels, gate run and gate apply in the level squelch's place, ahead of
    the tone squelch; lanes share setting and handles; reset_states reaches the gate's handle and reset() drops it."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    from radiocore.tools import audiofilter as af
    from radiocore.tools.gate import FrameGate

    class _Tensor(_FakeTensor):
        dtype = "f32"

        def data_ptr(self):
            return 0x100000

        def is_contiguous(self):
            return True

        def numel(self):
            return int(np.prod(self.shape))

    class _Torch(_FakeTorch):
        Tensor = _Tensor
        uint8 = "u8"
        int32 = "i32"

    fake = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: fake)
    monkeypatch.setattr(hip, "torch", lambda: _Torch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _Tensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_host", lambda x: x)
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _Tensor(getattr(x, "shape", (len(x),))))
    import radiocore as rc
    B, A, C = 12500, 8000, 4

    def tuner(channels=C):
        t = rc.Tuner()
        for i in range(channels):
            t.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
        t.request_bandwidth(600000.0)
        return t
    t = tuner()
    gate = FrameGate(frames=50)
    assert t._gate is None
    for bad in (dict(gate=None, open=1e-3), dict(gate=gate), dict(gate="gate", open=1e-3), dict(gate=gate, open=[1e-3] * 3),
                dict(gate=gate, open=1e-3, close=2e-3), dict(gate=gate, open=[1e-3] * C, close=[1e-3, 1e-3, 2e-3, 1e-3]),
                dict(gate=FrameGate(frames=64), open=1e-3),           # 64 divides A = 8000 but not B = 12 500
                dict(gate=FrameGate(frames=625), open=1e-3)):          # 625 divides B but not A
        with pytest.raises(ValueError):
            t.set_gate(**bad)
        assert t._gate is None
    t.set_squelch(1e-3)
    with pytest.raises(ValueError):
        t.set_gate(gate, open=1e-3)
    assert t._gate is None and t._squelch is not None
    t.set_squelch(None)
    t.set_gate(gate, open=[4e-3, 2e-3, 2e-3, 2e-3], hysteresis_db=3.0)
    held = t._gate
    assert held[1].dtype == np.float32 and held[2].dtype == np.float32
    assert np.allclose(held[2], held[1] * 10.0 ** -0.3, rtol=1e-6)
    with pytest.raises(ValueError):
        t.set_squelch(1e-3)
    with pytest.raises(ValueError):
        t.set_gate(FrameGate(frames=64), open=1e-3)
    assert t._gate is held and t._squelch is None
    assert fake.count("rcfm_gate_create") == 0
    t.set_tones(rc.ToneBank([100.0, 123.0], frame=2000), want=0, ratio=0.5)
    t.set_audio_filter(af.VOICE_NFM)
    t.load(np.zeros(600000, np.complex64))
    t.run_all()
    names = ("rcfm_pipeline_run", "rcfm_tone_bank_run", "rcfm_audio_filter_run", "rcfm_tuner_levels", "rcfm_tuner_frame_levels",
             "rcfm_gate_run", "rcfm_gate_apply", "rcfm_tone_score", "rcfm_squelch")
    order = [n for n, _ in fake.calls if n in names]
    assert order == ["rcfm_pipeline_run", "rcfm_tone_bank_run", "rcfm_audio_filter_run", "rcfm_tuner_frame_levels",
                     "rcfm_gate_run", "rcfm_gate_apply", "rcfm_tone_score", "rcfm_squelch"], order
    create = [a for n, a in fake.calls if n == "rcfm_gate_create"]
    assert len(create) == 1 and create[0][:3] == (C, 12, 1) and create[0][4] == 40
    levels = [a for n, a in fake.calls if n == "rcfm_tuner_frame_levels"][0]
    assert levels[1:4] == (0, C, 50) and levels[5].value == 8 * B * C
    run = [a for n, a in fake.calls if n == "rcfm_gate_run"][0]
    assert run[1:4] == (0, C, 50)
    apply = [a for n, a in fake.calls if n == "rcfm_gate_apply"][0]
    assert apply[2:6] == (C, 50, A, 1)
    t.set_tones(None)
    t.set_audio_filter(None)
    t.run_each()
    assert fake.count("rcfm_gate_create") == 1 and fake.count("rcfm_gate_run") == 2
    # frame_levels is a read: no gate needed, nothing but the one call
    plain = tuner()
    plain.load(np.zeros(600000, np.complex64))
    before = len(fake.calls)
    assert plain.frame_levels(50).shape == (C, 50)
    assert [n for n, _ in fake.calls[before:]] == ["rcfm_tuner_frame_levels"]
    with pytest.raises(ValueError):
        plain.frame_levels(64)
    with pytest.raises(ValueError):
        plain.frame_levels(0)
    # a lane shares the setting and the handles, with the fence on
    lane = t._lane_clone()
    assert lane._gate is t._gate and lane._gate_handles is t._gate_handles
    t._arm_state_fence()
    assert fake.count("rcfm_gate_set_fence") == 1
    t.reset_states()
    assert fake.count("rcfm_gate_reset") == 1
    # one more channel: the thresholds no longer fit -- refused by the next run before anything of it is launched
    before = fake.count("rcfm_pipeline_run")
    t.add_channel(446.0e6 + float(B) * C, B, rc.FM(B, A))
    t.load(np.zeros(600000, np.complex64))
    for call in (t.run_all, t.run_each):
        with pytest.raises(ValueError):
            call()
    assert fake.count("rcfm_pipeline_run") == before
    # ... and with one threshold for all channels the states move into a longer handle
    t.set_gate(gate, open=2e-3, close=1e-3)
    t.run_all()
    assert fake.count("rcfm_gate_create") == 2 and fake.count("rcfm_gate_get_state") == 1 and \
        fake.count("rcfm_gate_set_state") == 1 and fake.count("rcfm_gate_set_fence") == 2
    # another gate starts closed; None launches nothing more
    t.set_gate(FrameGate(frames=25), open=2e-3)
    assert not t._gate_handles
    t.set_gate(None)
    lane._sync_lane(t)
    assert lane._gate is None
    runs = fake.count("rcfm_gate_run") + fake.count("rcfm_tuner_frame_levels") + fake.count("rcfm_gate_apply")
    t.run_all()
    assert fake.count("rcfm_gate_run") + fake.count("rcfm_tuner_frame_levels") + fake.count("rcfm_gate_apply") == runs
    with pytest.raises(RuntimeError):
        t.frame_mask()
    # a gate set before the channels exist is checked by the first run
    late = rc.Tuner()
    late.set_gate(FrameGate(frames=64), open=1e-3)
    for i in range(C):
        late.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
    late.request_bandwidth(600000.0)
    late.load(np.zeros(600000, np.complex64))
    before = fake.count("rcfm_pipeline_run")
    for call in (late.run_all, late.run_each):
        with pytest.raises(ValueError):
            call()
    assert fake.count("rcfm_pipeline_run") == before
    with pytest.raises(ValueError):
        late.reset()
    assert not late._gate_handles
