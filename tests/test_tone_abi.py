"""The tone bank's entry points (include/rcfm.h: rcfm_tone_bank_create / _run / _destroy, rcfm_tone_score): declared,
exported, bound, and refusing every bad argument before any device call -- none of this needs a device.  The range of
`want` is the one thing the library cannot check (a device array): the Python layer does, and that is tested here too."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_tone_bank_create", "rcfm_tone_bank_run", "rcfm_tone_bank_destroy", "rcfm_tone_score")
ERR_SIZE, ERR_ARG = -1, -4
_vp, _i = ctypes.c_void_p, ctypes.c_int
_dp, _fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    lib.rcfm_tone_bank_create.argtypes = [_i, _dp, _i, _fp, ctypes.POINTER(_vp)]
    lib.rcfm_tone_bank_run.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]
    lib.rcfm_tone_bank_destroy.argtypes = [_vp]
    lib.rcfm_tone_score.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert [len(hip.SIGNATURES[n]) for n in NEW] == [5, 9, 1, 9]
    # the limits the Python layer and the GPU tests use are the kernels' own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "tones.h")).read()
    assert re.search(r"kToneMaxK\s*=\s*%d\b" % hip.RCFM_TONE_MAX_K, kernel)
    m = re.search(r"kToneSegChunks\s*=\s*(\d+)", kernel), re.search(r"kToneChunk\s*=\s*(\d+)", kernel)
    assert int(m[0].group(1)) * int(m[1].group(1)) == hip.RCFM_TONE_SEGMENT
    assert lib.rcfm_version() == 102


def _refused(lib, status, word, code=ERR_ARG):
    assert status == code, status
    assert word in lib.rcfm_last_error(), (word, lib.rcfm_last_error())


def _nu(*v):
    return (ctypes.c_double * len(v))(*v)


def _w(*v):
    return (ctypes.c_float * len(v))(*v)


def test_create_refuses_before_any_device_call(lib):
    out = _vp()
    create = lib.rcfm_tone_bank_create
    ok = _nu(0.01, 0.02)
    _refused(lib, create(2, None, 100, None, ctypes.byref(out)), b"NULL")
    _refused(lib, create(2, ok, 100, None, None), b"NULL")
    for K in (0, -1, 65):
        _refused(lib, create(K, _nu(*([0.1] * 65)), 100, None, ctypes.byref(out)), b"1 .. 64 tones")
    for L in (0, -5, (1 << 24) + 1):
        _refused(lib, create(2, ok, L, None, ctypes.byref(out)), b"frame length")
    for bad in (float("nan"), float("inf"), -1e-9, 0.5000001, -0.25):
        _refused(lib, create(2, _nu(0.1, bad), 100, None, ctypes.byref(out)), b"tone frequency")
    _refused(lib, create(1, _nu(0.1), 3, _w(1.0, float("nan"), 1.0), ctypes.byref(out)), b"window element")
    _refused(lib, create(1, _nu(0.1), 3, _w(1.0, float("inf"), 1.0), ctypes.byref(out)), b"window element")
    _refused(lib, create(1, _nu(0.1), 3, _w(1.0, -2.0, 1.0), ctypes.byref(out)), b"sum must be positive")
    _refused(lib, create(1, _nu(0.1), 3, _w(1.0, -1.0, -1.0), ctypes.byref(out)), b"sum must be positive")
    _refused(lib, create(1, _nu(0.1), 1, _w(0.0), ctypes.byref(out)), b"sum must be positive")     # the Hann window of one sample
    assert not out.value


def test_run_and_score_refuse_before_any_device_call(lib):
    p, odd = _vp(0x100000), _vp(0x100002)          # never dereferenced
    h = _vp(0x200000)                              # stands for a handle: every call below is refused before it is read
    run, score = lib.rcfm_tone_bank_run, lib.rcfm_tone_score
    _refused(lib, run(None, p, 1, 100, 1, 0, p, p, None), b"NULL")
    _refused(lib, run(h, None, 1, 100, 1, 0, p, p, None), b"NULL")
    _refused(lib, run(h, p, 1, 100, 1, 0, None, p, None), b"NULL")
    for count, A in ((0, 100), (-3, 100), (1, 0), (1, -1)):
        _refused(lib, run(h, p, count, A, 1, 0, p, p, None), b"at least 1")
    for step, offset in ((0, 0), (3, 0), (-1, 0), (1, 1), (1, -1), (2, 2), (2, -1)):
        _refused(lib, run(h, p, 1, 100, step, offset, p, p, None), b"step")
    for a, pw, e in ((odd, p, p), (p, odd, p), (p, p, odd)):
        _refused(lib, run(h, a, 1, 100, 1, 0, pw, e, None), b"misaligned")
    assert lib.rcfm_tone_bank_destroy(None) == 0
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        _refused(lib, score(a[0], a[1], a[2], None, 4, 2, 3, a[3], None), b"NULL")
    for count, F in ((0, 1), (-1, 1), (1, 0), (1, -2)):
        _refused(lib, score(p, p, p, None, count, F, 3, p, None), b"at least 1")
    for K in (0, -1, 65):
        _refused(lib, score(p, p, p, None, 4, 2, K, p, None), b"1 .. 64 tones")
    for a in ((odd, p, p, p), (p, odd, p, p), (p, p, odd, p), (p, p, p, odd)):
        _refused(lib, score(a[0], a[1], a[2], p, 4, 2, 3, a[3], None), b"misaligned")


def test_tone_bank_object_validates_on_the_host():
    """radiocore.ToneBank refuses what the library would refuse, without a device."""
    import radiocore as rc
    from radiocore.tools import tones
    for bad in (dict(freqs_hz=[]), dict(freqs_hz=np.arange(65.0)), dict(freqs_hz=[100.0, float("nan")]),
                dict(freqs_hz=[-1.0]), dict(freqs_hz=[100.0], frame=0), dict(freqs_hz=[100.0], window="hamming"),
                dict(freqs_hz=[100.0], frame=4, window=[1.0, 1.0, 1.0]), dict(freqs_hz=[[1.0, 2.0]])):
        with pytest.raises(ValueError):
            rc.ToneBank(**bad)
    bank = rc.ToneBank(tones.CTCSS)
    assert len(bank) == 39 and bank.frame is None
    assert bank.index(88.5) == 8 and bank.index(8) == 8 and bank.index(None) == -1 and bank.index(-1) == -1
    for bad in (39, -2, 88.4, 1000.0):
        with pytest.raises(ValueError):
            bank.index(bad)
    assert bank.frame_length(8000) == 8000 and rc.ToneBank([100.0], frame=160).frame_length(8000) == 160
    w = bank.window_array(8)
    assert w.dtype == np.float32 and w[0] == 0 and np.allclose(w, 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(8) / 8))
    assert rc.ToneBank([1.0], window="rect").window_array(8) is None


def test_set_tones_checks_want_on_the_host(monkeypatch):
    """`want` reaches rcfm_tone_score as a device array, which the library cannot validate: Tuner.set_tones checks its range
    (and everything else about the setting) before anything is uploaded.  Off by default."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    from radiocore.tools import tones
    fake = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: fake)
    monkeypatch.setattr(hip, "torch", lambda: _FakeTorch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _FakeTensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _FakeTensor(getattr(x, "shape", (len(x),))))
    import radiocore as rc
    B, A, C = 12500, 8000, 4
    tuner = rc.Tuner()
    for i in range(C):
        tuner.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
    assert tuner._tones is None
    with pytest.raises(RuntimeError):
        tuner.tone_power()
    bank = rc.ToneBank(tones.CTCSS)
    for bad in (dict(bank=None, want=3, ratio=0.01), dict(bank=bank, want=3), dict(bank=bank, ratio=0.01),
                dict(bank=bank, want=39, ratio=0.01), dict(bank=bank, want=-2, ratio=0.01),
                dict(bank=bank, want=[0, 1, 2], ratio=0.01), dict(bank=bank, want=[0, 1, 2, 64], ratio=0.01),
                dict(bank=bank, want=[0, 1, 2, 88.4], ratio=0.01), dict(bank=bank, want=3, ratio=[0.1, 0.2]),
                dict(bank=bank, want=3, ratio=np.ones((2, 2)))):
        with pytest.raises(ValueError):
            tuner.set_tones(**bad)
    assert tuner._tones is None
    tuner.set_tones(bank, want=[88.5, None, -1, 38], ratio=0.01)
    assert tuner._tones[1].dtype == np.int32 and tuner._tones[1].tolist() == [8, -1, -1, 38]
    assert tuner._tones[2].dtype == np.float32 and tuner._tones[2].tolist() == [np.float32(0.01)] * 4
    tuner.set_tones(bank)
    assert tuner._tones[1] is None and tuner._tones[2] is None
    # a bank that does not fit the channels' audio (A = 8000) is refused by set_tones, and the setting in force stays
    held = tuner._tones
    for misfit in (rc.ToneBank([100.0], frame=9000), rc.ToneBank([4000.5]), rc.ToneBank([100.0], window=np.ones(160, np.float32))):
        with pytest.raises(ValueError):
            tuner.set_tones(misfit)
        assert tuner._tones is held
    assert fake.count("rcfm_tone_bank_create") == 1          # the fitting bank's handle for A = 8000, made by set_tones
    # ... and where the channels come after the setting, by the next run before anything of it is launched
    late = rc.Tuner()
    late.set_tones(rc.ToneBank([100.0], frame=9000))
    for i in range(C):
        late.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
    late.request_bandwidth(600000.0)
    late.load(np.zeros(600000, np.complex64))
    for run in (late.run_all, late.run_each):
        with pytest.raises(ValueError):
            run()
    assert fake.count("rcfm_pipeline_run") == 0
    lane = tuner._lane_clone()
    assert lane._tones is tuner._tones
    tuner.set_tones(None)
    lane._sync_lane(tuner)
    assert tuner._tones is None and lane._tones is None
    assert not any(n in ("rcfm_tone_bank_run", "rcfm_tone_score") for n, _ in fake.calls)
