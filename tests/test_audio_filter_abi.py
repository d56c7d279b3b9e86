"""The audio filter's entry points (include/rcfm.h: rcfm_audio_filter_create / _run / _reset / _get_state / _set_state /
_set_fence / _destroy): declared, exported, bound, and refusing every bad argument before any device call -- none of
this needs a device.  RCFM_ERR_INDEX needs a handle, and a handle needs a device: tests/test_hip_audio_filter.py."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_audio_filter_create", "rcfm_audio_filter_run", "rcfm_audio_filter_reset", "rcfm_audio_filter_get_state",
       "rcfm_audio_filter_set_state", "rcfm_audio_filter_set_fence", "rcfm_audio_filter_destroy")
ERR_ARG = -4
_vp, _i = ctypes.c_void_p, ctypes.c_int
_dp = ctypes.POINTER(ctypes.c_double)
GOOD = (0.9, -1.8, 0.9, 1.0, -1.7, 0.75)                  # a stable section


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    lib.rcfm_audio_filter_create.argtypes = [_i, _i, _i, _dp, ctypes.POINTER(_vp)]
    lib.rcfm_audio_filter_run.argtypes = [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]
    lib.rcfm_audio_filter_reset.argtypes = [_vp, _vp]
    lib.rcfm_audio_filter_get_state.argtypes = [_vp, _dp, _vp]
    lib.rcfm_audio_filter_set_state.argtypes = [_vp, _dp, _vp]
    lib.rcfm_audio_filter_set_fence.argtypes = [_vp, _i]
    lib.rcfm_audio_filter_destroy.argtypes = [_vp]
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert re.search(r"typedef\s+struct\s+rcfm_audio_filter_s\s*\*\s*rcfm_audio_filter_t\s*;", header)
    assert [len(hip.SIGNATURES[n]) for n in NEW] == [5, 8, 2, 3, 3, 2, 1]
    # the limits the Python layer and the models use are the kernel's own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "audio_filter.h")).read()
    import sos_model
    for name, value in (("kSosMaxSections", hip.RCFM_SOS_MAX_SECTIONS), ("kSosRun", hip.RCFM_SOS_RUN),
                        ("kSosSegment", hip.RCFM_SOS_SEGMENT)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), kernel), name
    assert (sos_model.RUN, sos_model.SEGMENT) == (hip.RCFM_SOS_RUN, hip.RCFM_SOS_SEGMENT)
    assert hip.RCFM_SOS_RUN % 2 == 1
    assert lib.rcfm_version() == 102


def _refused(lib, status, word, code=ERR_ARG):
    assert status == code, status
    assert word in lib.rcfm_last_error(), (word, lib.rcfm_last_error())


def _sos(*rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_double * len(flat))(*flat)


def test_create_refuses_before_any_device_call(lib):
    out = _vp()
    create = lib.rcfm_audio_filter_create
    ok = _sos(GOOD)
    _refused(lib, create(1, 1, 1, None, ctypes.byref(out)), b"NULL")
    _refused(lib, create(1, 1, 1, ok, None), b"NULL")
    for C in (0, -1):
        _refused(lib, create(C, 1, 1, ok, ctypes.byref(out)), b"C must be at least 1")
    for ch in (0, 3, -1):
        _refused(lib, create(1, ch, 1, ok, ctypes.byref(out)), b"ch is 1 or 2")
    for S in (0, -1, 9):
        _refused(lib, create(1, 1, S, _sos(*([GOOD] * 9)), ctypes.byref(out)), b"1 .. 8 sections")
    for col in range(6):
        for bad in (float("nan"), float("inf"), -float("inf")):
            row = list(GOOD)
            row[col] = bad
            _refused(lib, create(1, 1, 2, _sos(GOOD, row), ctypes.byref(out)), b"not finite")
    for a0 in (0.0, 2.0, 1.0 + 2.0 ** -52, -1.0):
        _refused(lib, create(1, 1, 1, _sos((1.0, 0.0, 0.0, a0, -0.5, 0.0)), ctypes.byref(out)), b"a0 is not 1")
    # the stability triangle: |a2| < 1, |a1| < 1 + a2 -- its edges are refused
    for a1, a2 in ((0.0, 1.0), (0.0, -1.0), (0.0, 1.5), (2.0, 1.0), (1.5, 0.5), (-1.5, 0.5), (1.0, 0.0), (-1.0, 0.0),
                   (-1.9987, 0.9986), (0.5, -0.5), (0.25, -0.75)):
        _refused(lib, create(1, 2, 2, _sos(GOOD, (1.0, 0.0, 0.0, 1.0, a1, a2)), ctypes.byref(out)), b"not strictly stable")
    assert not out.value


def test_the_other_entry_points_refuse_before_any_device_call(lib):
    p, odd = _vp(0x100000), _vp(0x100002)          # never dereferenced
    h = _vp(0x200000)                              # stands for a handle: every call below is refused before it is read
    run = lib.rcfm_audio_filter_run
    _refused(lib, run(None, 0, 1, 100, p, p, None, None), b"NULL")
    _refused(lib, run(h, 0, 1, 100, None, p, None, None), b"NULL")
    _refused(lib, run(h, 0, 1, 100, p, None, None, None), b"NULL")
    for count, n in ((0, 100), (-3, 100), (1, 0), (1, -1)):
        _refused(lib, run(h, 0, count, n, p, p, None, None), b"at least 1")
    for a, b in ((odd, p), (p, odd)):
        _refused(lib, run(h, 0, 1, 100, a, b, None, None), b"misaligned")
    state = (ctypes.c_double * 4)()
    _refused(lib, lib.rcfm_audio_filter_reset(None, None), b"NULL")
    _refused(lib, lib.rcfm_audio_filter_get_state(None, state, None), b"NULL")
    _refused(lib, lib.rcfm_audio_filter_get_state(h, None, None), b"NULL")
    _refused(lib, lib.rcfm_audio_filter_set_state(None, state, None), b"NULL")
    _refused(lib, lib.rcfm_audio_filter_set_state(h, None, None), b"NULL")
    _refused(lib, lib.rcfm_audio_filter_set_fence(None, 1), b"NULL")
    assert lib.rcfm_audio_filter_destroy(None) == 0


def test_the_python_layer_refuses_what_the_library_refuses():
    """radiocore.AudioFilter checks a design before it reaches rcfm_audio_filter_create: the same triangle."""
    from radiocore.tools.audiofilter import AudioFilter
    for a1, a2 in ((0.0, 1.0), (1.5, 0.5), (-1.0, 0.0), (0.5, -0.5)):
        with pytest.raises(ValueError):
            AudioFilter.sos([[1.0, 0.0, 0.0, 1.0, a1, a2]], 8000)
    assert AudioFilter.sos([GOOD], 8000).sections(8000).tolist() == [list(GOOD)]
    import sos_model
    for rate in (8000, 48000):                     # the hard case of the GPU tests is inside the triangle
        assert AudioFilter.sos(sos_model.elliptic(rate), rate).sections(rate).shape == (8, 6)


def test_set_audio_filter_on_the_host(monkeypatch):
    """Tuner.set_audio_filter: off by default, refusals with the setting in force kept, for channels added later in the next
    run before anything is launched; the run queues the filter between the tone bank and the squelch; lanes share setting
    and handles; reset_states reaches the filter's handle and reset() drops it."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    from radiocore.tools import audiofilter as af
    class _Tensor(_FakeTensor):
        def data_ptr(self):
            return 0x100000

        def numel(self):
            return int(np.prod(self.shape))

    class _Torch(_FakeTorch):
        Tensor = _Tensor
        uint8 = "u8"

    fake = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: fake)
    monkeypatch.setattr(hip, "torch", lambda: _Torch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _Tensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_host", lambda x: x)
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _Tensor(getattr(x, "shape", (len(x),))))
    import radiocore as rc
    assert rc.AudioFilter is af.AudioFilter
    B, A, C = 12500, 8000, 4

    def tuner(channels=C):
        t = rc.Tuner()
        for i in range(channels):
            t.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
        t.request_bandwidth(600000.0)
        return t
    t = tuner()
    assert t._afilt is None
    for bad in (dict(filt=None, channels=[True] * C), dict(filt=af.VOICE_NFM, channels=[True] * 3),
                dict(filt=af.VOICE_NFM, channels=np.ones((2, 2), bool)), dict(filt="voice"),
                dict(filt=af.AudioFilter.lowpass(4000.0)), dict(filt=af.AudioFilter.sos([GOOD], 48000))):
        with pytest.raises(ValueError):
            t.set_audio_filter(**bad)
        assert t._afilt is None
    t.set_audio_filter(af.VOICE_NFM, channels=[True, False, True, True])
    held = t._afilt
    assert held[1].dtype == np.uint8 and held[1].tolist() == [1, 0, 1, 1]
    with pytest.raises(ValueError):
        t.set_audio_filter(af.AudioFilter.lowpass(4000.0))
    assert t._afilt is held
    assert fake.count("rcfm_audio_filter_create") == 0
    t.set_squelch(1e-3)
    t.load(np.zeros(600000, np.complex64))
    t.run_all()
    order = [n for n, _ in fake.calls if n in ("rcfm_pipeline_run", "rcfm_audio_filter_run", "rcfm_tuner_levels", "rcfm_squelch")]
    assert order == ["rcfm_pipeline_run", "rcfm_audio_filter_run", "rcfm_tuner_levels", "rcfm_squelch"], order
    create = [a for n, a in fake.calls if n == "rcfm_audio_filter_create"]
    assert len(create) == 1 and create[0][:3] == (C, 1, 5)
    run = [a for n, a in fake.calls if n == "rcfm_audio_filter_run"][0]
    assert run[1:4] == (0, C, A) and run[4].value == run[5].value
    t.run_each()
    assert fake.count("rcfm_audio_filter_create") == 1 and fake.count("rcfm_audio_filter_run") == 2
    # a lane shares the setting and the handles, with the fence on
    lane = t._lane_clone()
    assert lane._afilt is t._afilt and lane._afilt_handles is t._afilt_handles
    t._arm_state_fence()
    assert fake.count("rcfm_audio_filter_set_fence") == 1
    t.reset_states()
    assert fake.count("rcfm_audio_filter_reset") == 1
    # one more channel: the selection no longer fits -- refused by the next run before anything of it is launched
    before = fake.count("rcfm_pipeline_run")
    t.add_channel(446.0e6 + float(B) * C, B, rc.FM(B, A))
    t.load(np.zeros(600000, np.complex64))
    for call in (t.run_all, t.run_each):
        with pytest.raises(ValueError):
            call()
    assert fake.count("rcfm_pipeline_run") == before
    # ... and with a setting for all channels the states move into a longer handle
    t.set_audio_filter(af.VOICE_NFM)
    t.run_all()
    assert fake.count("rcfm_audio_filter_create") == 2 and fake.count("rcfm_audio_filter_get_state") == 1 and \
        fake.count("rcfm_audio_filter_set_state") == 1 and fake.count("rcfm_audio_filter_set_fence") == 2
    # another filter starts at rest; None launches nothing more
    t.set_audio_filter(af.VOICE_AM)
    assert not t._afilt_handles
    t.set_audio_filter(None)
    lane._sync_lane(t)
    assert lane._afilt is None
    runs = fake.count("rcfm_audio_filter_run")
    t.run_all()
    assert fake.count("rcfm_audio_filter_run") == runs
    # a filter set before the channels exist is checked by the first run
    late = rc.Tuner()
    late.set_audio_filter(af.AudioFilter.lowpass(4000.0))
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
    assert not late._afilt_handles
