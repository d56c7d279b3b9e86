"""The IQ balance entry points (include/rcfm.h: rcfm_tuner_iq_estimate, rcfm_tuner_iq_correct, rcfm_tuner_set_iq_balance):
declared, exported, bound, and refusing bad arguments before any device call.  What can be refused without a handle is
checked on the CPU (those checks come first and name what they refuse); the refusals that depend on the handle's n need a
tuner handle and so a device, and still come before anything is launched.  Plus the validation of Tuner.set_iq_balance."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_tuner_iq_estimate", "rcfm_tuner_iq_correct", "rcfm_tuner_set_iq_balance")
_f = ctypes.c_float
_i64 = ctypes.c_int64
ERR_ARG, ERR_STATE = -4, -5
OFF, FIXED, AUTO = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    lib.rcfm_tuner_iq_estimate.argtypes = [ctypes.c_void_p, _i64, _i64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.rcfm_tuner_iq_correct.argtypes = [ctypes.c_void_p, ctypes.c_void_p, _i64, ctypes.c_void_p]
    lib.rcfm_tuner_set_iq_balance.argtypes = [ctypes.c_void_p, ctypes.c_int, _f, _f, _i64]
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert [len(hip.SIGNATURES[n]) for n in NEW] == [6, 4, 5]
    for name, value in (("OFF", 0), ("FIXED", 1), ("AUTO", 2)):
        assert re.search(r"RCFM_IQ_BALANCE_%s\s*=\s*%d\b" % (name, value), header)
        assert getattr(hip, "RCFM_IQ_BALANCE_" + name) == value
    # the segment geometry the GPU tests straddle is the kernels' own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "iq_balance.h")).read()
    assert re.search(r"kIqSegPairs\s*=\s*%d\b" % hip.RCFM_IQ_SEG_PAIRS, kernel)
    assert re.search(r"kIqMaxSegs\s*=\s*%d\b" % hip.RCFM_IQ_MAX_SEGS, kernel)
    assert lib.rcfm_version() == 102


def _refused(lib, status, word):
    assert status == ERR_ARG, status
    assert word in lib.rcfm_last_error(), (word, lib.rcfm_last_error())


def test_refusals_that_need_no_handle(lib):
    """A NULL handle, and everything that is wrong whatever the handle: refused on the host, the handle-independent checks
    first (so their message, not "NULL handle", comes back for a NULL handle too)."""
    p = ctypes.c_void_p(0x100000)          # never dereferenced
    est, cor, setb = lib.rcfm_tuner_iq_estimate, lib.rcfm_tuner_iq_correct, lib.rcfm_tuner_set_iq_balance
    _refused(lib, est(None, 1, 10, p, p, None), b"NULL handle")
    _refused(lib, est(None, 1, 10, None, None, None), b"both outputs")
    for m_lo, m_hi in ((0, 10), (-1, 10), (5, 4), (1, 0)):
        _refused(lib, est(None, m_lo, m_hi, p, p, None), b"empty pair range")
    _refused(lib, cor(None, p, 0, None), b"NULL handle")
    _refused(lib, cor(None, None, 0, None), b"beta is NULL")
    _refused(lib, cor(None, p, -1, None), b"negative dc_notch")
    _refused(lib, setb(None, OFF, _f(0), _f(0), 0), b"NULL handle")
    _refused(lib, setb(None, AUTO, _f(0), _f(0), 0), b"NULL handle")
    for mode in (-1, 3, 7):
        _refused(lib, setb(None, mode, _f(0), _f(0), 0), b"unknown balance mode")
    _refused(lib, setb(None, AUTO, _f(0), _f(0), -1), b"negative dc_notch")
    for re_, im in ((float("nan"), 0.0), (0.0, float("inf")), (float("-inf"), 0.0)):
        _refused(lib, setb(None, FIXED, _f(re_), _f(im), 0), b"not finite")
    for re_, im in ((1.0, 0.0), (0.0, -1.0), (0.8, 0.6), (3.0, 4.0)):
        _refused(lib, setb(None, FIXED, _f(re_), _f(im), 0), b"below 1")
    _refused(lib, setb(None, FIXED, _f(0.6), _f(0.6), 0), b"NULL handle")       # |beta| = 0.85: fine, the handle is not
    _refused(lib, setb(None, AUTO, _f(float("nan")), _f(9.0), 0), b"NULL handle")   # beta is ignored outside fixed mode


@pytest.mark.gpu
@pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")
def test_refusals_that_depend_on_the_handle(lib):
    """Out-of-range pairs (every n < 3 has none), a notch beyond n / 2, and the call order: all before any launch."""
    from radiocore._internal import hip
    rt = hip.lib()
    p = ctypes.c_void_p(0x100000)          # never dereferenced: every call below is refused on the host

    def tuner(n):
        h = ctypes.c_void_p()
        hip.check(rt.rcfm_tuner_create(n, 0, None, None, ctypes.byref(h)))
        return hip.Handle(h, rt.rcfm_tuner_destroy)
    for n, last in ((1, 0), (2, 0), (3, 1), (4, 1), (90001, 45000), (600000, 299999)):
        t = tuner(n)
        _refused(rt, rt.rcfm_tuner_iq_estimate(t.value, 1, last + 1, p, p, None), b"pair range")
        _refused(rt, rt.rcfm_tuner_iq_estimate(t.value, last + 1, last + 1, p, p, None), b"pair range")
        _refused(rt, rt.rcfm_tuner_iq_correct(t.value, p, n // 2 + 1, None), b"dc_notch")
        _refused(rt, rt.rcfm_tuner_set_iq_balance(t.value, FIXED, _f(0.01), _f(0.0), n // 2 + 1), b"dc_notch")
        if n < 3:
            _refused(rt, rt.rcfm_tuner_iq_estimate(t.value, 1, 1, p, p, None), b"pair range")
            _refused(rt, rt.rcfm_tuner_set_iq_balance(t.value, AUTO, _f(0), _f(0), 0), b"fewer than 3")
        else:
            # in range, but nothing is loaded: the state is refused next, still before any launch
            assert rt.rcfm_tuner_iq_estimate(t.value, 1, last, p, p, None) == ERR_STATE
            assert rt.rcfm_tuner_iq_correct(t.value, p, n // 2, None) == ERR_STATE
            assert rt.rcfm_tuner_set_iq_balance(t.value, AUTO, _f(0), _f(0), n // 2) == 0
            assert rt.rcfm_tuner_set_iq_balance(t.value, OFF, _f(0), _f(0), 0) == 0


def test_set_iq_balance_validates_like_the_abi_and_follows_the_handle(monkeypatch):
    """The Python layer with the ABI replaced by a counting stand-in: ValueError for whatever the library would refuse;
    off by default (no call at all); a setting made before the first load reaches the handle when it is built, a later one
    at once; a lane takes the base tuner's setting with its next load."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    fake = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: fake)
    monkeypatch.setattr(hip, "torch", lambda: _FakeTorch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _FakeTensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _FakeTensor(getattr(x, "shape", (len(x),))))
    import radiocore as rc
    B, A, C, N = 25000, 8000, 4, 600_000
    tuner = rc.Tuner()
    for i in range(C):
        tuner.add_channel(118.0e6 + float(B) * i, B, rc.AM(B, A))
    tuner.request_bandwidth(float(N))
    for bad in (dict(balance="blind"), dict(balance=1.0 + 0j), dict(balance=0.8 + 0.6j), dict(balance=complex("nan")),
                dict(balance=complex(0.0, float("inf"))), dict(balance="auto", dc_notch=-1), dict(balance=0.01j, dc_notch=-2),
                dict(balance="auto", dc_notch=N // 2 + 1), dict(balance=[1, 2])):
        with pytest.raises(ValueError):
            tuner.set_iq_balance(**bad)
    x = np.zeros(N, np.complex64)
    tuner.load(x)
    assert fake.count("rcfm_tuner_set_iq_balance") == 0                  # off by default: not even a call
    tuner.set_iq_balance("auto", dc_notch=1)
    calls = [a for n, a in fake.calls if n == "rcfm_tuner_set_iq_balance"]
    assert len(calls) == 1 and tuple(calls[0][1:]) == (hip.RCFM_IQ_BALANCE_AUTO, 0.0, 0.0, 1)
    tuner.load(x)
    assert fake.count("rcfm_tuner_set_iq_balance") == 1                  # the handle has it already
    beta = complex(np.float32(-0.0237), np.float32(-0.0268))
    tuner.set_iq_balance(beta, dc_notch=3)
    last = [a for n, a in fake.calls if n == "rcfm_tuner_set_iq_balance"][-1]
    assert tuple(last[1:]) == (hip.RCFM_IQ_BALANCE_FIXED, beta.real, beta.imag, 3)
    lane = tuner._lane_clone()
    before = fake.count("rcfm_tuner_set_iq_balance")
    lane.load(x)                                                         # a new handle: set when it is built
    assert fake.count("rcfm_tuner_set_iq_balance") == before + 1
    tuner.set_iq_balance(None)
    lane._sync_lane(tuner)
    lane.load(x)
    last = [a for n, a in fake.calls if n == "rcfm_tuner_set_iq_balance"][-1]
    assert last[1] == hip.RCFM_IQ_BALANCE_OFF
    # a setting made before the first load of a fresh tuner travels with the handle's creation
    fresh = rc.Tuner()
    fresh.add_channel(118.0e6, B, rc.AM(B, A))
    fresh.request_bandwidth(float(N))
    fresh.set_iq_balance("auto")
    before = fake.count("rcfm_tuner_set_iq_balance")
    fresh.load(x)
    assert fake.count("rcfm_tuner_set_iq_balance") == before + 1
