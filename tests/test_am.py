"""CPU: the AM demodulator's surface (include/rcfm.h RCFM_AM, radiocore.AM, Tuner bookkeeping) -- librcfm.so loaded,
no device used."""

import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "rcfm.h")


@pytest.fixture(scope="module")
def hip():
    from radiocore._internal import hip
    hip.lib()
    return hip


def test_kind_in_the_header_and_the_binding(hip):
    m = re.search(r"\bRCFM_AM\s*=\s*(\d+)", open(HEADER).read())
    assert m is not None and int(m.group(1)) == 3
    assert hip.RCFM_AM == 3
    assert (hip.RCFM_FM, hip.RCFM_MFM, hip.RCFM_WBFM) == (0, 1, 2)


def test_create_checks_sizes_before_the_device(hip):
    lib = hip.lib()
    h = ctypes.c_void_p()
    assert lib.rcfm_demod_create(3, 1, 100, 0, ctypes.c_double(75e-6), 0, ctypes.byref(h)) == -4
    assert b"bad demodulator size" in lib.rcfm_last_error()
    assert lib.rcfm_demod_create(4, 1, 100, 50, ctypes.c_double(75e-6), 0, ctypes.byref(h)) == -4
    assert b"kind" in lib.rcfm_last_error()


class _FakeTensor:
    is_cuda = True

    def __init__(self, shape):
        self.shape = tuple(shape)

    def __getitem__(self, k):
        return self


class _FakeTorch:
    complex64 = "c64"
    float32 = "f32"
    Tensor = _FakeTensor


class _CountingLib:
    """librcfm stand-in: every entry point returns 0 and records its arguments; *_create hands out a handle."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name.endswith("_create"):
                args[-1]._obj.value = 0x1000 + len(self.calls)
            return 0
        return fn

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


@pytest.fixture()
def no_device(monkeypatch):
    """The package's Python layer without a device: torch and the ABI replaced by stand-ins (no compute call)."""
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


def test_class_surface(no_device):
    import radiocore
    from radiocore import AM
    from radiocore.analog import AM as AM2
    assert AM is AM2 is radiocore.analog.am.AM
    am = AM(25000, 8000)
    assert am.channels == 1
    assert AM(25000, 8000, deemphasis=50e-6, batch=4).channels == 1
    for bad in [dict(input_size=1, output_size=8000), dict(input_size=25000, output_size=0),
                dict(input_size=25000, output_size=8000, batch=0)]:
        with pytest.raises(ValueError):
            AM(**bad)


def _tuner(kinds, B=25000, A=8000):
    import radiocore as rc
    t = rc.Tuner()
    for i, k in enumerate(kinds):
        t.add_channel(100e6 + 25000.0 * i, B, getattr(rc, k)(B, A))
    t.request_bandwidth(2_000_000.0)
    return t


def test_tuner_geometry_and_plan(no_device):
    import radiocore as rc
    from radiocore._internal import hip
    from radiocore.tools.tuner import Tuner
    assert Tuner._geometry(rc.AM(25000, 8000)) == (3, 25000, 8000, 75e-6)
    t = _tuner(["AM"] * 3 + ["MFM"] * 2 + ["AM"] * 2)
    groups, first, count = t._launch_plan()
    assert (first, count) == (0, 7)
    assert [g[:3] for g in groups] == [(0, 3, hip.RCFM_AM), (3, 2, hip.RCFM_MFM), (5, 2, hip.RCFM_AM)]
    assert t._plan_uniform() is None
    assert _tuner(["AM"] * 4)._plan_uniform() == (hip.RCFM_AM, 25000, 8000, 75e-6)


def test_run_all_refuses_am_next_to_fm(no_device):
    t = _tuner(["AM", "FM", "AM"])
    t.load(np.zeros(2_000_000, np.complex64))
    with pytest.raises(ValueError, match="one demodulator class and geometry"):
        t.run_all()


def test_am_groups_need_no_state_binding(no_device):
    """run_each over AM | MFM | AM: the MFM group binds its channels' state and arms the Lanes fence; the AM groups
    (a stateless kind, like FM) do neither, and AM's one-channel objects stay unbound."""
    from radiocore._internal import hip
    lib = no_device
    t = _tuner(["AM"] * 3 + ["MFM"] * 2 + ["AM"] * 2)
    t.load(np.zeros(2_000_000, np.complex64))
    out = t.run_each()
    assert len(out) == 7
    kinds = [args[0] for n, args in lib.calls if n == "rcfm_demod_create"]
    assert sorted(kinds) == [hip.RCFM_MFM, hip.RCFM_AM]          # one batched handle per geometry
    assert lib.count("rcfm_pipeline_run") == 3
    assert [c.demodulator._binding is None for c in t.channels()] == [True] * 3 + [False] * 2 + [True] * 2
    assert all(k[0] == hip.RCFM_MFM for k in t._state_owner)
    lib.calls.clear()
    t._arm_state_fence()
    fenced = [args for n, args in lib.calls if n == "rcfm_demod_set_option" and args[1] == hip.RCFM_OPT_STATE_FENCE]
    assert len(fenced) == 1                                     # the MFM handle only
    lib.calls.clear()
    assert t.run_each() and lib.count("rcfm_demod_bind_state") == 0
