"""The noise floor's entry points (include/rcfm.h: rcfm_rank_filter, rcfm_floor_create / _run / _thresholds / _reset /
_get_state / _set_state / _set_fence / _destroy): declared, exported, bound, and refusing every bad argument before any device
call -- none of this needs a device -- and Tuner.set_floor / OverFloor on the host.  What needs a handle needs a device:
tests/test_hip_floor.py."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_rank_filter", "rcfm_floor_create", "rcfm_floor_run", "rcfm_floor_thresholds", "rcfm_floor_reset",
       "rcfm_floor_get_state", "rcfm_floor_set_state", "rcfm_floor_set_fence", "rcfm_floor_destroy")
ERR_ARG = -4
_vp, _i, _i64, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_fp = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    lib.rcfm_rank_filter.argtypes = [_vp, _i64, _i, _i, _i, _vp, _vp]
    lib.rcfm_floor_create.argtypes = [_i64, _i, _i, _i, _f, _f, ctypes.POINTER(_vp)]
    lib.rcfm_floor_run.argtypes = [_vp, _vp, _f, _vp, _vp, _vp]
    lib.rcfm_floor_thresholds.argtypes = [_vp, _i64, _vp, _vp, _i, _vp, _vp]
    lib.rcfm_floor_reset.argtypes = [_vp, _vp]
    lib.rcfm_floor_get_state.argtypes = [_vp, _fp, _vp]
    lib.rcfm_floor_set_state.argtypes = [_vp, _fp, _vp]
    lib.rcfm_floor_set_fence.argtypes = [_vp, _i]
    lib.rcfm_floor_destroy.argtypes = [_vp]
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert re.search(r"typedef\s+struct\s+rcfm_floor_s\s*\*\s*rcfm_floor_t\s*;", header)
    assert [len(hip.SIGNATURES[n]) for n in NEW] == [7, 7, 6, 7, 2, 3, 3, 2, 1]
    # the limits the Python layer uses are the kernel's own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "floor.h")).read()
    assert re.search(r"kFloorMaxHalf\s*=\s*%d\b" % hip.RCFM_FLOOR_MAX_HALF, kernel)
    assert re.search(r"kFloorMaxCells\s*=\s*\(int64_t\)1\s*<<\s*30\b", kernel) and hip.RCFM_FLOOR_MAX_CELLS == 1 << 30
    assert lib.rcfm_version() == 102
    # no profile stage was added: the list still ends with the squelch's
    lib.rcfm_profile_stage_name.restype = ctypes.c_char_p
    lib.rcfm_profile_stage_name.argtypes = [_i]
    assert lib.rcfm_profile_stage_name(lib.rcfm_profile_stage_count() - 1) == b"squelch"


def _refused(lib, status, word, code=ERR_ARG):
    assert status == code, status
    assert word in lib.rcfm_last_error(), (word, lib.rcfm_last_error())


def _window_refusals(lib, call):
    """call(M, half, guard, q): the refusals rcfm_rank_filter and rcfm_floor_create share."""
    for half in (0, -1, 4097):
        _refused(lib, call(1000, half, 0, 250), b"half outside")
    for half, guard in ((64, -1), (64, 64), (1, 1), (4096, 4096)):
        _refused(lib, call(10000, half, guard, 250), b"guard outside")
    for q in (-1, 1001):
        _refused(lib, call(1000, 64, 4, q), b"q outside")
    for M, guard in ((1, 0), (0, 0), (-5, 0), (5, 4), (13, 12)):
        _refused(lib, call(M, 64, guard, 250), b"below guard + 2")
    _refused(lib, call(2 ** 30 + 1, 64, 4, 250), b"above 2^30")


def test_rank_filter_refuses_before_any_device_call(lib):
    p, p2, odd = _vp(0x100000), _vp(0x200000), _vp(0x100002)          # never dereferenced
    rf = lib.rcfm_rank_filter
    _refused(lib, rf(None, 1000, 64, 4, 250, p2, None), b"NULL")
    _refused(lib, rf(p, 1000, 64, 4, 250, None, None), b"NULL")
    _refused(lib, rf(p, 1000, 64, 4, 250, p, None), b"out must not be x")
    _window_refusals(lib, lambda M, half, guard, q: rf(p, M, half, guard, q, p2, None))
    _refused(lib, rf(odd, 1000, 64, 4, 250, p2, None), b"misaligned")
    _refused(lib, rf(p, 1000, 64, 4, 250, odd, None), b"misaligned")


def test_floor_create_refuses_before_any_device_call(lib):
    out = _vp()
    create = lib.rcfm_floor_create
    _refused(lib, create(1000, 64, 4, 250, 0.1, 0.6, None), b"NULL")
    _window_refusals(lib, lambda M, half, guard, q: create(M, half, guard, q, 0.1, 0.6, ctypes.byref(out)))
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        _refused(lib, create(1000, 64, 4, 250, bad, 0.6, ctypes.byref(out)), b"rise is not in (0, 1]")
        _refused(lib, create(1000, 64, 4, 250, 0.1, bad, ctypes.byref(out)), b"fall is not in (0, 1]")
    assert not out.value


def test_the_other_entry_points_refuse_before_any_device_call(lib):
    p, p2, odd = _vp(0x100000), _vp(0x300000), _vp(0x100002)          # never dereferenced
    h = _vp(0x200000)                              # stands for a handle: every call below is refused before it is read
    run, thr = lib.rcfm_floor_run, lib.rcfm_floor_thresholds
    _refused(lib, run(None, p, 2.0, p2, p2, None), b"NULL")
    _refused(lib, run(h, None, 2.0, p2, p2, None), b"NULL")
    _refused(lib, run(h, p, 2.0, None, None, None), b"both NULL")
    _refused(lib, run(h, p, 2.0, p, None, None), b"floor must not be power")
    _refused(lib, run(h, p, float("nan"), p2, None, None), b"ratio is NaN")
    _refused(lib, run(h, odd, 2.0, p2, None, None), b"misaligned")
    _refused(lib, run(h, p, 2.0, odd, None, None), b"misaligned")
    for k in range(4):                             # floor, cell, gain, thr
        args = [p, p, p, p2]
        args[k] = None
        _refused(lib, thr(args[0], 100, args[1], args[2], 4, args[3], None), b"NULL")
        args[k] = odd
        _refused(lib, thr(args[0], 100, args[1], args[2], 4, args[3], None), b"misaligned")
    for M in (0, -1, 2 ** 30 + 1):
        _refused(lib, thr(p, M, p, p, 4, p2, None), b"M outside")
    _refused(lib, thr(p, 100, p, p, -1, p2, None), b"negative channel count")
    assert thr(p, 100, p, p, 0, p2, None) == 0                               # no channels: nothing is launched
    state = (ctypes.c_float * 2)()
    _refused(lib, lib.rcfm_floor_reset(None, None), b"NULL")
    _refused(lib, lib.rcfm_floor_get_state(None, state, None), b"NULL")
    _refused(lib, lib.rcfm_floor_get_state(h, None, None), b"NULL")
    _refused(lib, lib.rcfm_floor_set_state(None, state, None), b"NULL")
    _refused(lib, lib.rcfm_floor_set_state(h, None, None), b"NULL")
    _refused(lib, lib.rcfm_floor_set_fence(None, 1), b"NULL")
    assert lib.rcfm_floor_destroy(None) == 0


def test_set_floor_on_the_host(monkeypatch):
    """Tuner.set_floor: off by default and then nothing new is queued; with a floor every load queues power spectrum, floor
    run and thresholds behind the library's load; OverFloor stands where squelch and gate take a threshold and is refused
    without a floor, the setting in force kept; lanes share setting and handle, with the fence on; reset_states reaches the
    handle, reset() and another NoiseFloor drop it; shard and attached spectra are refused."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    from radiocore.tools.floor import NoiseFloor, OverFloor
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
    uploads = []
    monkeypatch.setattr(hip, "lib", lambda: fake)
    monkeypatch.setattr(hip, "torch", lambda: _Torch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _Tensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_host", lambda x: x)

    def to_device(x, dtype=None):
        uploads.append(np.array(x))
        return _Tensor(getattr(x, "shape", (len(x),)))
    monkeypatch.setattr(hip, "to_device", to_device)
    import radiocore as rc
    assert rc.NoiseFloor is NoiseFloor and rc.OverFloor is OverFloor
    B, A, C, N = 12500, 8000, 4, 600000
    FLOOR = ("rcfm_tuner_power_spectrum", "rcfm_floor_create", "rcfm_floor_run", "rcfm_floor_thresholds", "rcfm_floor_reset",
             "rcfm_floor_set_fence", "rcfm_floor_get_state", "rcfm_floor_set_state")

    def tuner(channels=C):
        t = rc.Tuner()
        for i in range(channels):
            t.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
        t.request_bandwidth(float(N))
        return t
    t = tuner()
    x = np.zeros(N, np.complex64)
    # off by default: a load and a run queue nothing of the floor's
    assert t._floor is None
    t.set_squelch(1e-3)
    t.load(x)
    t.run_all()
    assert not [n for n, _ in fake.calls if n in FLOOR]
    for read in (t.floor, t.floor_levels, lambda: t.occupied_cells(6.0)):
        with pytest.raises(RuntimeError):
            read()
    # OverFloor without a floor: refused, the setting in force stays
    held = t._squelch
    with pytest.raises(ValueError):
        t.set_squelch(OverFloor(10))
    assert t._squelch is held
    t.set_squelch(None)
    with pytest.raises(ValueError):
        t.set_gate(FrameGate(frames=50), open=OverFloor(10))
    assert t._gate is None
    for bad in ("floor", 3.0, OverFloor(3)):
        with pytest.raises(ValueError):
            t.set_floor(bad)
    with pytest.raises(ValueError):
        t.set_floor(NoiseFloor(200000.0, half=8, guard=4))          # 3 cells: fewer than guard + 2
    assert t._floor is None
    # with a floor: three calls behind the load, in order, over the whole band
    nf = NoiseFloor(1000.0, half=40, guard=8, quantile=0.25)
    t.set_floor(nf)
    t.set_squelch(OverFloor(10))
    before = len(fake.calls)
    uploads.clear()
    t.load(x)
    order = [n for n, _ in fake.calls[before:] if n in FLOOR or n == "rcfm_tuner_load"]
    assert order == ["rcfm_tuner_load", "rcfm_tuner_power_spectrum", "rcfm_floor_create", "rcfm_floor_run", "rcfm_floor_thresholds"]
    ps = [a for n, a in fake.calls[before:] if n == "rcfm_tuner_power_spectrum"][0]
    assert ps[1:4] == (-(N // 2), N, 600) and ps[5] is None
    create = [a for n, a in fake.calls if n == "rcfm_floor_create"][0]
    assert create[:4] == (600, 40, 8, 250) and abs(create[4] - (1.0 - np.exp(-0.1))) < 1e-7 and abs(create[5] - (1.0 - np.exp(-1.0))) < 1e-7
    thr = [a for n, a in fake.calls[before:] if n == "rcfm_floor_thresholds"][0]
    assert thr[1] == 600 and thr[4] == 2 * C                        # 0 dB (floor_levels) and the squelch's 10 dB
    # the tables: the cell of every channel's centre bin, and G / len(cell) 10^(db / 10)
    cell, gain = [u for u in uploads if u.shape == (2 * C,)]
    centre = np.array([int(round(ch.center_frequency - t.input_frequency)) + N // 2 for ch in t.channels()])
    assert cell.dtype == np.int32 and cell.tolist() == (centre // 1000).tolist() * 2
    from radiocore.tools.floor import channel_noise_gain
    G = channel_noise_gain(B, N)
    assert gain.dtype == np.float32 and np.allclose(gain[:C], G / 1000.0, rtol=1e-7) and np.allclose(gain[C:], 10.0 * G / 1000.0, rtol=1e-7)
    # the squelch compares against the load's thresholds: no upload, no further floor call
    before = len(fake.calls)
    uploads.clear()
    t.run_all()
    assert [n for n, _ in fake.calls[before:] if n in ("rcfm_tuner_levels", "rcfm_squelch") or n in FLOOR] == ["rcfm_tuner_levels", "rcfm_squelch"]
    assert not uploads
    # a figure set after the load gets its thresholds from the load's floor: one more stateless call, no second floor run
    t.set_squelch(OverFloor(6))
    t.run_all()
    assert fake.count("rcfm_floor_thresholds") == 2 and fake.count("rcfm_floor_run") == 1
    # the next load uses the same handle; reads need no further call
    t.load(x)
    assert fake.count("rcfm_floor_create") == 1 and fake.count("rcfm_floor_run") == 2
    calls = len(fake.calls)
    assert t.floor().shape == (600,) and t.floor_levels() is not None and len(fake.calls) == calls
    # the gate takes OverFloor for both thresholds; close defaults to open lowered by the hysteresis
    t.set_squelch(None)
    gate = FrameGate(frames=50)
    for bad in (dict(open=OverFloor(10), close=1e-3), dict(open=1e-3, close=OverFloor(3)), dict(open=OverFloor(5), close=OverFloor(6))):
        with pytest.raises(ValueError):
            t.set_gate(gate, **bad)
        assert t._gate is None
    t.set_gate(gate, open=OverFloor(10), hysteresis_db=4.0)
    assert (t._gate[1].db, t._gate[2].db) == (10.0, 6.0)
    t.set_gate(gate, open=OverFloor(10), close=OverFloor(7))
    before = len(fake.calls)
    t.load(x)
    assert [a for n, a in fake.calls[before:] if n == "rcfm_floor_thresholds"][0][4] == 3 * C
    t.run_all()
    assert fake.count("rcfm_gate_run") == 1
    # while an OverFloor is in force the floor cannot go
    with pytest.raises(ValueError):
        t.set_floor(None)
    assert t._floor is nf
    # a lane shares the setting and the handle, with the fence on
    lane = t._lane_clone()
    assert lane._floor is nf and lane._floor_handles is t._floor_handles
    t._arm_state_fence()
    assert fake.count("rcfm_floor_set_fence") == 1
    t.reset_states()
    assert fake.count("rcfm_floor_reset") == 1
    # another NoiseFloor drops the handle: no cell is primed; the lane follows
    nf2 = NoiseFloor(1000.0, half=40, guard=8, quantile=0.5)
    t.set_floor(nf2)
    assert not t._floor_handles
    lane._sync_lane(t)
    assert lane._floor is nf2
    lane.load(x)
    assert fake.count("rcfm_floor_create") == 2 and fake.count("rcfm_floor_set_fence") == 2      # made by the lane, fenced, shared
    t.load(x)
    assert fake.count("rcfm_floor_create") == 2
    # off again: nothing more of the floor's
    t.set_gate(None)
    t.set_floor(None)
    assert not t._floor_handles
    before = len(fake.calls)
    t.load(x)
    t.run_all()
    assert not [n for n, _ in fake.calls[before:] if n in FLOOR]
    # the floor needs the whole spectrum
    t.set_floor(nf)
    t.shard(0, 2)
    with pytest.raises(RuntimeError):
        t.load(x)
    sharded = tuner()
    sharded.shard(0, 2)
    with pytest.raises(ValueError):
        sharded.set_floor(nf)
    assert sharded._floor is None
    # reset() drops the handle with the channels
    other = tuner()
    other.set_floor(nf)
    other.load(x)
    assert other._floor_handles
    with pytest.raises(ValueError):
        other.reset()
    assert not other._floor_handles
