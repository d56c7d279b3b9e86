"""CPU: the AGC's entry points (include/rcfm.h: rcfm_agc, rcfm_demod_set_agc, rcfm_demod_get / set_agc_state) -- declared,
exported, bound, and refusing bad arguments before any device call -- and the Python surface (radiocore.AGC, the `agc`
keyword of AM / USB / LSB, the Tuner's bookkeeping) with the ABI replaced by a counting stand-in."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_am import _CountingLib, _FakeTensor, _FakeTorch  # noqa: F401  (the same stand-ins as the AM surface tests)

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_agc", "rcfm_demod_set_agc", "rcfm_demod_get_agc_state", "rcfm_demod_set_agc_state")
_f = ctypes.c_float
_d = ctypes.c_double


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert len(hip.SIGNATURES["rcfm_agc"]) == 10 and len(hip.SIGNATURES["rcfm_demod_set_agc"]) == 4
    assert re.search(r"RCFM_AGC_PEAK\s*=\s*0\b", header) and re.search(r"RCFM_AGC_CARRIER\s*=\s*1\b", header)
    assert (hip.RCFM_AGC_PEAK, hip.RCFM_AGC_CARRIER) == (0, 1)
    assert lib.rcfm_version() == 102


def test_rcfm_agc_refuses_bad_arguments_without_a_device(lib):
    p = ctypes.c_void_p(0x1000)        # never dereferenced: every call below is refused on the host
    q = ctypes.c_void_p(0x100000)

    def call(C=3, n=100, mode=0, decay=2400.0, level=0.25, floor=0.0, state=p, v=q, audio=q):
        return lib.rcfm_agc(C, n, mode, _d(decay), _f(level), _f(floor), state, v, audio, None)
    bad = [dict(mode=2), dict(mode=-1), dict(decay=0.0), dict(decay=-1.0), dict(decay=float("nan")), dict(decay=float("inf")),
           dict(level=0.0), dict(level=-0.25), dict(level=float("nan")), dict(level=float("inf")),
           dict(floor=-1e-9), dict(floor=float("nan")), dict(floor=float("inf")),
           dict(C=0), dict(C=65536), dict(n=0), dict(state=None), dict(v=None), dict(audio=None),
           dict(audio=ctypes.c_void_p(0x100000 + 4)),            # partial overlap: one sample on
           dict(audio=ctypes.c_void_p(0x100000 + 4 * 150))]      # ... and from the middle of the second row
    for kw in bad:
        assert call(**kw) == -4, kw
    lib.rcfm_last_error.restype = ctypes.c_char_p
    assert call(C=65536) == -4 and b"65535" in lib.rcfm_last_error()
    assert call(audio=ctypes.c_void_p(0x100000 + 4)) == -4 and b"overlap" in lib.rcfm_last_error()


def test_demod_entry_points_refuse_null_without_a_device(lib):
    assert lib.rcfm_demod_set_agc(None, _d(2400.0), _f(0.25), _f(0.0)) == -4
    buf = (ctypes.c_float * 4)()
    assert lib.rcfm_demod_get_agc_state(None, buf, None) == -4
    assert lib.rcfm_demod_set_agc_state(None, buf, None) == -4


def test_profile_stages_did_not_move(lib):
    """The AGC tail is timed as the stage of the kernel it replaces: the list of stages is what it was."""
    lib.rcfm_profile_stage_name.restype = ctypes.c_char_p
    names = [lib.rcfm_profile_stage_name(i).decode() for i in range(lib.rcfm_profile_stage_count())]
    assert names[-4:] == ["am_tail", "ssb_tail", "levels", "squelch"]


# ---- the Python surface ------------------------------------------------------------------------------------------------

@pytest.fixture()
def no_device(monkeypatch):
    from radiocore._internal import hip
    lib = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: lib)
    monkeypatch.setattr(hip, "torch", lambda: _FakeTorch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _FakeTensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _FakeTensor(getattr(x, "shape", (len(x),))))
    monkeypatch.setattr(hip, "to_host", lambda x: x)
    return lib


def test_agc_class_and_keyword(no_device):
    import radiocore as rc
    from radiocore.analog import AGC
    assert rc.AGC is AGC
    a = rc.AGC()
    assert (a.decay, a.level, a.floor) == (0.3, None, 0.0) and a == rc.AGC(0.3) and a != rc.AGC(0.2)
    assert rc.AM(25000, 8000, agc=a)._agc == (0.3 * 8000, 1.0, 0.0)
    assert rc.USB(12500, 8000, agc=a)._agc == (0.3 * 8000, 0.25, 0.0)
    assert rc.LSB(12500, 48000, agc=rc.AGC(0.5, level=0.1, floor=1e-3))._agc == (0.5 * 48000, 0.1, 1e-3)
    assert rc.AM(25000, 8000)._agc is None and rc.USB(12500, 8000, agc=None)._agc is None
    for bad in (dict(decay=0.0), dict(decay=-1.0), dict(decay=float("nan")), dict(level=0.0), dict(level=float("inf")),
                dict(floor=-1.0), dict(floor=float("nan"))):
        with pytest.raises(ValueError):
            rc.AGC(**bad)
    with pytest.raises(ValueError):
        rc.USB(12500, 8000, agc=0.3)
    for cls in (rc.FM, rc.MFM, rc.WBFM):
        with pytest.raises(TypeError):
            cls(240000, 48000, agc=a)
    with pytest.raises(ValueError):
        rc.AM(25000, 8000).agc_state()


def test_handle_sets_the_agc_before_it_binds(no_device):
    import radiocore as rc
    lib = no_device
    d = rc.USB(12500, 8000, agc=rc.AGC(0.3, floor=0.01))
    d.run(np.zeros(12500, np.complex64))
    names = [n for n, _ in lib.calls]
    assert names.index("rcfm_demod_set_agc") == names.index("rcfm_demod_create") + 1
    args = [a for n, a in lib.calls if n == "rcfm_demod_set_agc"][0]
    assert tuple(args[1:]) == (2400.0, 0.25, 0.01)
    lib.calls.clear()
    rc.USB(12500, 8000).run(np.zeros(12500, np.complex64))
    assert lib.count("rcfm_demod_set_agc") == 0


def _tuner(specs, B=25000, A=8000):
    import radiocore as rc
    t = rc.Tuner()
    for i, (k, agc) in enumerate(specs):
        t.add_channel(118.0e6 + float(B) * i, B, getattr(rc, k)(B, A, **({"agc": agc} if agc is not None else {})))
    t.request_bandwidth(600_000.0)
    return t


def test_tuner_groups_bind_and_fence_by_agc_setting(no_device):
    import radiocore as rc
    from radiocore._internal import hip
    from radiocore.tools.tuner import Tuner
    lib = no_device
    a, b = rc.AGC(0.3, floor=0.01), rc.AGC(0.1, floor=0.01)
    assert Tuner._geometry(rc.AM(25000, 8000)) == (3, 25000, 8000, 75e-6)            # off: today's key
    assert Tuner._geometry(rc.AM(25000, 8000, agc=a)) == (3, 25000, 8000, 75e-6, (2400.0, 1.0, 0.01))
    t = _tuner([("AM", None)] * 2 + [("AM", a)] * 2 + [("AM", rc.AGC(0.3, floor=0.01))] + [("AM", b)] + [("USB", a)] * 2
               + [("USB", None)])
    groups, first, count = t._launch_plan()
    assert [g[:3] for g in groups] == [(0, 2, 3), (2, 3, 3), (5, 1, 3), (6, 2, 5), (8, 1, 5)]
    assert [len(g) for g in groups] == [6, 7, 7, 7, 6]
    assert t._plan_uniform() is None
    t.load(np.zeros(600_000, np.complex64))
    assert len(t.run_each()) == 9
    assert lib.count("rcfm_demod_create") == 5 and lib.count("rcfm_demod_set_agc") == 3 and lib.count("rcfm_pipeline_run") == 5
    bound = [c.demodulator._binding is not None for c in t.channels()]
    assert bound == [False] * 2 + [True] * 6 + [False]
    assert len(t._state_owner) == 3 and all(len(k) == 6 for k in t._state_owner)
    lib.calls.clear()
    t._arm_state_fence()
    fenced = [args for n, args in lib.calls if n == "rcfm_demod_set_option" and args[1] == hip.RCFM_OPT_STATE_FENCE]
    assert len(fenced) == 3
    lib.calls.clear()
    t.reset_states()
    assert lib.count("rcfm_demod_reset_state") == 5
    u = _tuner([("USB", a)] * 4)
    assert u._plan_uniform() == (5, 25000, 8000, 75e-6, (2400.0, 0.25, 0.01))
    u.load(np.zeros(600_000, np.complex64))
    lib.calls.clear()
    u.run_all()
    assert lib.count("rcfm_demod_set_agc") == 1 and lib.count("rcfm_pipeline_run") == 1
