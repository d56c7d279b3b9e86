"""CPU: the noise blanker's entry points (include/rcfm.h: rcfm_blanker_create / _run / _destroy; include/rcfm_tools.h:
rcfm_blanker_last) are declared, exported and bound; what create refuses is refused before any device call; and every
ValueError of NoiseBlanker and Tuner.set_blanker comes without a device."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
ERR_ARG = -4


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from radiocore._internal import hip
    return hip.load_library(LIB)


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    host, tools = _header("rcfm.h"), _header("rcfm_tools.h")
    for name in ("rcfm_blanker_create", "rcfm_blanker_run", "rcfm_blanker_destroy"):
        assert re.search(r"\bint\s+%s\s*\(" % name, host), name
    assert re.search(r"\bint\s+rcfm_blanker_last\s*\(", tools) and "rcfm_blanker_last" not in host
    assert re.search(r"typedef\s+struct\s+rcfm_blanker\s*\*\s*rcfm_blanker_t\s*;", host)
    for name, argc in (("rcfm_blanker_create", 9), ("rcfm_blanker_run", 7), ("rcfm_blanker_destroy", 1), ("rcfm_blanker_last", 4)):
        assert hasattr(lib, name) and len(hip.SIGNATURES[name]) == argc, name
    assert re.search(r"RCFM_BLANK_MEDIAN\s*=\s*0\b", host) and re.search(r"RCFM_BLANK_ABSOLUTE\s*=\s*1\b", host)
    assert re.search(r"RCFM_IQ_CF32\s*=\s*0\b", host)
    assert (hip.RCFM_BLANK_MEDIAN, hip.RCFM_BLANK_ABSOLUTE, hip.RCFM_IQ_CF32) == (0, 1, 0)
    # the limits the Python layer refuses by are the kernels' own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "blanker.h")).read()
    assert re.search(r"kBlankMinBlock\s*=\s*%d\b" % hip.RCFM_BLANK_MIN_BLOCK, kernel)
    assert re.search(r"kBlankMaxBlockLog2\s*=\s*%d\b" % (hip.RCFM_BLANK_MAX_BLOCK.bit_length() - 1), kernel)
    assert re.search(r"kBlankMaxSpan\s*=\s*%d\b" % hip.RCFM_BLANK_MAX_SPAN, kernel)
    assert re.search(r"kBlankMaxGuard\s*=\s*%d\b" % hip.RCFM_BLANK_MAX_GUARD, kernel)


def test_the_load_entry_points_still_refuse_format_0(lib):
    p = ctypes.c_void_p(0x100000)          # never dereferenced
    assert lib.rcfm_iq_convert(0, 16, p, p, None) == ERR_ARG
    assert b"unknown IQ format" in lib.rcfm_last_error()
    assert lib.rcfm_tuner_load_raw(None, 0, p, None) == ERR_ARG


def test_create_and_run_refuse_before_any_device_call(lib):
    out = ctypes.c_void_p()
    ramp = (ctypes.c_float * 4)(0.2, 0.4, 0.6, 0.8)
    ok = dict(n_max=100000, block=4096, span=4, mode=0, value=15.8, hold=2, ramp_host=ramp, ramp=4)

    def create(**kw):
        a = dict(ok, **kw)
        return lib.rcfm_blanker_create(a["n_max"], a["block"], a["span"], a["mode"], a["value"], a["hold"], a["ramp_host"],
                                       a["ramp"], kw.get("out", ctypes.byref(out)))

    bad_ramps = [(ctypes.c_float * 4)(0.2, v, 0.6, 0.8) for v in (-0.01, 1.01, float("nan"), float("inf"))]
    for kw, word in [(dict(out=None), b"NULL"), (dict(n_max=0), b"n_max"), (dict(n_max=-5), b"n_max"), (dict(n_max=(1 << 40) + 1), b"n_max"),
                     (dict(block=0), b"block"), (dict(block=32), b"block"), (dict(block=96), b"block"), (dict(block=4095), b"block"),
                     (dict(block=1 << 21), b"block"), (dict(block=-64), b"block"),
                     (dict(span=-1), b"half-span"), (dict(span=9), b"half-span"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
                     (dict(value=0.0), b"value"), (dict(value=-1.0), b"value"), (dict(value=float("nan")), b"value"),
                     (dict(value=float("inf")), b"value"),
                     (dict(hold=-1), b"hold"), (dict(ramp=-1), b"hold"), (dict(hold=1021), b"hold"), (dict(hold=1 << 30), b"hold"),
                     (dict(hold=0, ramp=1025), b"hold"), (dict(ramp_host=None), b"NULL ramp")] + \
                    [(dict(ramp_host=r), b"ramp value") for r in bad_ramps]:
        assert create(**kw) == ERR_ARG, kw
        assert word in lib.rcfm_last_error(), (kw, lib.rcfm_last_error())
    p = ctypes.c_void_p(0x100000)
    assert lib.rcfm_blanker_run(None, 0, 16, p, p, None, None) == ERR_ARG and b"NULL handle" in lib.rcfm_last_error()
    assert lib.rcfm_blanker_last(None, None, None, None) == ERR_ARG
    assert lib.rcfm_blanker_destroy(None) == 0


def test_noise_blanker_validates_without_a_device():
    import radiocore as rc
    from radiocore._internal import hip
    for bad in (dict(threshold_db=float("nan")), dict(threshold_db=float("inf")), dict(threshold_db=4000.0), dict(hold=-1e-6),
                dict(ramp=-1e-6), dict(hold=float("nan")), dict(ramp=float("inf")), dict(block=0), dict(block=32), dict(block=100),
                dict(block=1 << 21), dict(span=-1), dict(span=9), dict(absolute=0.0), dict(absolute=-1.0),
                dict(absolute=float("nan")), dict(absolute=float("inf"))):
        with pytest.raises(ValueError):
            rc.NoiseBlanker(**bad)
    nb = rc.NoiseBlanker()
    assert (nb.mode, nb.block, nb.span) == (hip.RCFM_BLANK_MEDIAN, 4096, 4) and abs(nb.value - 10.0 ** 1.2) < 1e-12
    assert rc.NoiseBlanker(absolute=0.5).mode == hip.RCFM_BLANK_ABSOLUTE and rc.NoiseBlanker(absolute=0.5).value == 0.5
    # hold and ramp are seconds of a one-second buffer
    H, ramp = nb.geometry(20_000_000)
    assert H == 40 and ramp.shape == (20,) and ramp.dtype == np.float32
    j = np.arange(20, dtype=np.float64)
    assert np.array_equal(ramp, (0.5 * (1.0 - np.cos(np.pi * (j + 1.0) / 21.0))).astype(np.float32))
    assert np.all(np.diff(ramp) > 0) and 0.0 < ramp[0] and ramp[-1] < 1.0
    assert nb.geometry(240_000)[0] == 0 and nb.geometry(240_000)[1].shape == (0,)
    with pytest.raises(ValueError):
        nb.geometry(400_000_000)                   # 800 + 400 samples
    with pytest.raises(ValueError):
        nb.geometry(-1)
    # buffers: refused by dtype and shape, before torch or the library are looked at
    assert nb.describe(np.zeros(10, np.complex64)) == (hip.RCFM_IQ_CF32, 10)
    assert nb.describe(np.zeros(10, np.complex128)) == (hip.RCFM_IQ_CF32, 10)
    assert nb.describe(np.zeros((10, 2), np.int16)) == (hip.RCFM_IQ_CS16, 10)
    assert nb.describe(np.zeros(20, np.int8)) == (hip.RCFM_IQ_CS8, 10)
    assert nb.describe(np.zeros((10, 2), np.uint8)) == (hip.RCFM_IQ_CU8, 10)
    for bad in (np.zeros(10, np.float32), np.zeros((10, 2), np.int32), np.zeros((2, 10), np.complex64), np.zeros(11, np.int16),
                np.zeros((10, 3), np.uint8), np.zeros((5, 2, 2), np.int8)):
        with pytest.raises(ValueError):
            nb.run(bad)
    with pytest.raises(ValueError):
        rc.NoiseBlanker(hold=1e-3).run(np.zeros(2_000_000, np.complex64))


def test_set_blanker_validates_is_off_by_default_and_follows_the_lanes(monkeypatch):
    """The Python layer with the ABI replaced by a counting stand-in: nothing of the blanker is called by default; with one set
    every load queues one run ahead of the library's load, in place on the upload; a lane makes a handle of its own."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    fake = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: fake)
    monkeypatch.setattr(hip, "torch", lambda: _FakeTorch)
    monkeypatch.setattr(_FakeTorch, "int64", "i64", raising=False)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _FakeTensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _FakeTensor(getattr(x, "shape", (len(x),))))
    import radiocore as rc
    B, A, N = 25000, 8000, 600_000
    tuner = rc.Tuner()
    for i in range(4):
        tuner.add_channel(118.0e6 + float(B) * i, B, rc.AM(B, A))
    tuner.request_bandwidth(float(N))
    x = np.zeros(N, np.complex64)
    tuner.load(x)
    assert not [n for n, _ in fake.calls if "blanker" in n]                # off by default: not even a call
    for bad in ("auto", 12.0, object()):
        with pytest.raises(ValueError):
            tuner.set_blanker(bad)
    with pytest.raises(ValueError):
        tuner.set_blanker(rc.NoiseBlanker(hold=1e-3, ramp=1e-3))          # 1200 samples of this tuner's buffers
    with pytest.raises(RuntimeError):
        tuner.blanker_stats()
    nb = rc.NoiseBlanker(hold=1e-5, ramp=1e-5)
    tuner.set_blanker(nb)
    tuner.load(x)
    tuner.load(x)
    names = [n for n, _ in fake.calls]
    assert names.count("rcfm_blanker_create") == 1 and names.count("rcfm_blanker_run") == 2
    create = [a for n, a in fake.calls if n == "rcfm_blanker_create"][0]
    assert tuple(create[:6]) == (N, 4096, 4, hip.RCFM_BLANK_MEDIAN, nb.value, 6) and create[7] == 6
    assert names[-2:] == ["rcfm_blanker_run", "rcfm_tuner_load"]
    run = [a for n, a in fake.calls if n == "rcfm_blanker_run"][-1]
    assert (run[1], run[2]) == (hip.RCFM_IQ_CF32, N)
    lane = tuner._lane_clone()
    lane.load(x)
    assert [n for n, _ in fake.calls].count("rcfm_blanker_create") == 2   # the lane's own handle and scratch
    assert lane._blank_handles[N][1] is not tuner._blank_handles[N][1]
    tuner.set_blanker(None)
    lane._sync_lane(tuner)
    before = len(fake.calls)
    tuner.load(x)
    lane.load(x)
    assert not [n for n, _ in fake.calls[before:] if "blanker" in n]
