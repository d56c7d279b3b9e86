"""The bus dynamics' entry points (include/rcfm.h: rcfm_busdyn_create / _run / _reset / _set_fence / _destroy; rcfm_tools.h:
rcfm_busdyn_state): declared, exported, bound, and refusing every bad argument before any device call -- none of this needs
a device -- and Tuner.set_bus_dynamics on the host, against a library that counts its calls.  What needs a handle needs a
device (A above the handle's A_max and partly overlapping buffers among it): tests/test_hip_busdyn.py."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_busdyn_create", "rcfm_busdyn_run", "rcfm_busdyn_reset", "rcfm_busdyn_set_fence", "rcfm_busdyn_destroy")
TOOLS = ("rcfm_busdyn_state",)
ERR_ARG = -4
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_ip, _fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    lib.rcfm_busdyn_create.argtypes = [_i, _i, _i, _i, _f, _f, _ip, _fp, _fp, _ip, ctypes.POINTER(_vp)]
    lib.rcfm_busdyn_run.argtypes = [_vp, _i, _vp, _vp, _vp, _vp, _vp]
    lib.rcfm_busdyn_reset.argtypes = [_vp, _vp]
    lib.rcfm_busdyn_set_fence.argtypes = [_vp, _i]
    lib.rcfm_busdyn_state.argtypes = [_vp, _fp, _fp, _ip]
    lib.rcfm_busdyn_destroy.argtypes = [_vp]
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip

    def header(name):
        return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    for names, text in ((NEW, header("rcfm.h")), (TOOLS, header("rcfm_tools.h"))):
        for name in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, text), name
            assert hasattr(lib, name), name
            assert name in hip.SIGNATURES, name
    assert not re.search(r"rcfm_busdyn_state", header("rcfm.h"))
    assert re.search(r"typedef\s+struct\s+rcfm_busdyn_s\s*\*\s*rcfm_busdyn_t\s*;", header("rcfm.h"))
    assert [len(hip.SIGNATURES[n]) for n in NEW + TOOLS] == [11, 7, 2, 2, 1, 4]
    # the prototypes' parameter counts in the header are the bound ones
    for names, text in ((NEW, header("rcfm.h")), (TOOLS, header("rcfm_tools.h"))):
        for name in names:
            params = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text).group(1)
            assert len(params.split(",")) == len(hip.SIGNATURES[name]), name
    # the limits the Python layer uses are the kernel's own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "busdyn.h")).read()
    assert re.search(r"kBusdynMaxBuses\s*=\s*%d\b" % hip.RCFM_BUSDYN_MAX_BUSES, kernel)
    assert re.search(r"kBusdynMinBlock\s*=\s*%d\b" % hip.RCFM_BUSDYN_MIN_BLOCK, kernel) and hip.RCFM_BUSDYN_MIN_BLOCK == 8
    assert re.search(r"kBusdynMaxBlock\s*=\s*%d\b" % hip.RCFM_BUSDYN_MAX_BLOCK, kernel) and hip.RCFM_BUSDYN_MAX_BLOCK == 2048
    assert re.search(r"kBusdynMaxHold\s*=\s*1\s*<<\s*15\b", kernel) and hip.RCFM_BUSDYN_MAX_HOLD == 1 << 15
    assert lib.rcfm_version() == 102
    # no profile stage was added: the list still ends with the squelch's
    lib.rcfm_profile_stage_name.restype = ctypes.c_char_p
    lib.rcfm_profile_stage_name.argtypes = [_i]
    assert lib.rcfm_profile_stage_name(lib.rcfm_profile_stage_count() - 1) == b"squelch"


def _refused(lib, status, word):
    assert status == ERR_ARG, status
    assert word in lib.rcfm_last_error(), (word, lib.rcfm_last_error())


def _tables(key, depth, thr, hold):
    keep = (np.ascontiguousarray(key, dtype=np.int32), np.ascontiguousarray(depth, dtype=np.float32),
            np.ascontiguousarray(thr, dtype=np.float32), np.ascontiguousarray(hold, dtype=np.int32))
    return keep, (keep[0].ctypes.data_as(_ip), keep[1].ctypes.data_as(_fp), keep[2].ctypes.data_as(_fp), keep[3].ctypes.data_as(_ip))


def test_create_refuses_before_any_device_call(lib):
    out = _vp()
    create = lib.rcfm_busdyn_create
    none = (None, None, None, None)
    _refused(lib, create(2, 2, 64, 8000, 0.9, 0.1, *none, None), b"NULL")
    for M in (0, -1, 1025):
        _refused(lib, create(M, 2, 64, 8000, 0.9, 0.1, *none, ctypes.byref(out)), b"M outside")
    for ch in (0, 3, -1):
        _refused(lib, create(2, ch, 64, 8000, 0.9, 0.1, *none, ctypes.byref(out)), b"ch outside")
    for L in (7, 0, -64, 2049):
        _refused(lib, create(2, 2, L, 8000, 0.9, 0.1, *none, ctypes.byref(out)), b"L outside")
    for A_max in (0, -1, (1 << 30) + 1):
        _refused(lib, create(2, 2, 64, A_max, 0.9, 0.1, *none, ctypes.byref(out)), b"A_max outside")
    for c in (0.0, -0.5, np.nan, np.inf, -np.inf):
        _refused(lib, create(2, 2, 64, 8000, c, 0.1, *none, ctypes.byref(out)), b"ceiling")
    for k in (0.0, -0.1, 1.0000001, np.nan, np.inf):
        _refused(lib, create(2, 2, 64, 8000, 0.9, k, *none, ctypes.byref(out)), b"release_k outside")
    good = ([1, -1, 0], [0.5, 1.0, 0.25], [0.01, 0.0, 0.3], [3, 0, 1 << 15])
    keep, t = _tables(*good)
    for missing in (1, 2, 3):
        _refused(lib, create(3, 2, 64, 8000, 0.9, 0.1, *[None if i == missing else p for i, p in enumerate(t)], ctypes.byref(out)),
                 b"NULL")

    def with_(column, m, value):
        cols = [list(c) for c in good]
        cols[column][m] = value
        return _tables(*cols)
    for bad in (-2, 3, 100):
        keep, t = with_(0, 0, bad)
        _refused(lib, create(3, 2, 64, 8000, 0.9, 0.1, *t, ctypes.byref(out)), b"key is outside")
    for m in range(3):
        keep, t = with_(0, m, m)
        _refused(lib, create(3, 2, 64, 8000, 0.9, 0.1, *t, ctypes.byref(out)), b"its own key")
    for bad in (0.0, -0.5, 1.5, np.nan, np.inf):
        keep, t = with_(1, 2, bad)
        _refused(lib, create(3, 2, 64, 8000, 0.9, 0.1, *t, ctypes.byref(out)), b"depth is outside")
    for bad in (-0.001, np.nan, -np.inf):
        keep, t = with_(2, 0, bad)
        _refused(lib, create(3, 2, 64, 8000, 0.9, 0.1, *t, ctypes.byref(out)), b"threshold")
    for bad in (-1, (1 << 15) + 1):
        keep, t = with_(3, 1, bad)
        _refused(lib, create(3, 2, 64, 8000, 0.9, 0.1, *t, ctypes.byref(out)), b"hold is outside")
    assert not out.value
    assert lib.rcfm_busdyn_destroy(None) == 0


def test_run_and_the_rest_refuse_before_any_device_call(lib):
    p, p2, odd = _vp(0x100000), _vp(0x900000), _vp(0x100002)          # never dereferenced
    h = _vp(0x200000)                              # stands for a handle: every call below is refused before it is read
    run = lib.rcfm_busdyn_run
    _refused(lib, run(None, 100, p, None, p2, None, None), b"NULL")
    _refused(lib, run(h, 100, None, None, p2, None, None), b"NULL")
    _refused(lib, run(h, 100, p, None, None, None, None), b"NULL")
    for A in (0, -5):
        _refused(lib, run(h, A, p, None, p2, None, None), b"A below 1")
    _refused(lib, run(h, 100, odd, None, p2, None, None), b"misaligned")
    _refused(lib, run(h, 100, p, None, odd, None, None), b"misaligned")
    _refused(lib, run(h, 100, p, None, p, None, None), b"out overlaps in")
    _refused(lib, lib.rcfm_busdyn_reset(None, None), b"NULL")
    _refused(lib, lib.rcfm_busdyn_set_fence(None, 1), b"NULL")
    _refused(lib, lib.rcfm_busdyn_state(None, None, None, None), b"NULL")


def test_settings_objects_and_duck_resolution():
    import radiocore as rc
    from radiocore.tools import busdyn
    assert rc.Limiter is busdyn.Limiter and rc.Duck is busdyn.Duck
    lim = rc.Limiter()
    assert (lim.ceiling_db, lim.lookahead, lim.release) == (-1.0, 0.008, 0.25)
    d = rc.Duck("tower")
    assert (d.key, d.depth_db, d.threshold_db, d.hold) == ("tower", -12.0, -40.0, 0.5)
    buses = [rc.Bus.of([0], name="tower"), rc.Bus.of([1], name="rest"), rc.Bus.of([2])]
    key, per = busdyn.resolve_ducks({"rest": d, 2: rc.Duck(1)}, buses)
    assert key.tolist() == [-1, 0, 1] and per[0] is None and per[1] is d
    for bad in ({"nobody": d}, {"rest": rc.Duck("nobody")}, {0: rc.Duck(0)}, {"tower": d}, {3: d}, {-1: d}, {"rest": "duck"},
                {1: d, "rest": rc.Duck(2)}, {1.5: d}):
        with pytest.raises(ValueError):
            busdyn.resolve_ducks(bad, buses)
    with pytest.raises(ValueError):
        busdyn.resolve_ducks({"twin": rc.Duck(0)}, [rc.Bus.of([0]), rc.Bus.of([1], name="twin"), rc.Bus.of([2], name="twin")])


def test_set_bus_dynamics_on_the_host(monkeypatch):
    """Tuner.set_bus_dynamics: off by default and then no rcfm_busdyn_* call; set, rcfm_busdyn_run follows rcfm_mix_run of its
    group on the mixer's rows and mask; one handle per group, kept while the audio lengths stay; a duck across groups is
    refused before anything is launched; lanes share setting and handles; reset_states resets, reset() drops."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip

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
    DYN = ("rcfm_busdyn_create", "rcfm_busdyn_run", "rcfm_busdyn_reset", "rcfm_busdyn_set_fence", "rcfm_busdyn_destroy")

    def tuner(channels=C, wide=0):
        t = rc.Tuner()
        for i in range(channels):
            t.add_channel(446.0e6 + float(B) * i, B, rc.FM(B, A))
        for i in range(wide):                       # a second launch group: another bandwidth
            t.add_channel(446.0e6 + float(B) * channels + 25000.0 * i + 6250.0, 25000, rc.FM(25000, A))
        t.request_bandwidth(float(N))
        return t

    def dyn_calls(since=0):
        return [(n, a) for n, a in fake.calls[since:] if n in DYN]
    t = tuner()
    x = np.zeros(N, np.complex64)
    tower, rest = rc.Bus.of([1, 3], name="tower"), rc.Bus.of([0, 2, 4, 5], gain_db=-6.0, name="rest")
    mixer = rc.Mixer([tower, rest])
    # needs a mixer first; the setting in force stays
    with pytest.raises(ValueError, match="mixer"):
        t.set_bus_dynamics(rc.Limiter())
    t.set_mix(mixer)
    t.set_squelch(1e-3)
    t.load(x)
    t.run_all()
    assert not dyn_calls() and t._busdyn is None and t.bus_delay() == [0]
    for bad in (dict(limiter="limiter"), dict(ducks={"rest": rc.Duck("tower")}), dict(limiter=rc.Limiter(), ducks={"rest": rc.Duck("nobody")}),
                dict(limiter=rc.Limiter(), ducks={"tower": rc.Duck("tower")}), dict(limiter=rc.Limiter(), ducks={2: rc.Duck(0)})):
        with pytest.raises(ValueError):
            t.set_bus_dynamics(**bad)
    assert t._busdyn is None and not dyn_calls()
    # set: one create, and the run follows the group's mixer on its rows and mask
    t.set_bus_dynamics(rc.Limiter(), ducks={"rest": rc.Duck("tower")})
    before = len(fake.calls)
    t.run_all()
    names = [n for n, _ in fake.calls[before:]]
    assert names.count("rcfm_busdyn_create") == 1 and names.count("rcfm_busdyn_run") == 1
    assert names.index("rcfm_mix_run") + 1 == names.index("rcfm_busdyn_run") == len(names) - 1
    create = [a for n, a in dyn_calls(before) if n == "rcfm_busdyn_create"][0]
    assert create[:4] == (2, 2, 64, A)
    assert np.float32(create[4]) == np.float32(10.0 ** -0.05) and np.float32(create[5]) == np.float32(1.0 - np.exp(-64 / 2000.0))
    assert [create[6][m] for m in range(2)] == [-1, 0] and create[9][1] == 62
    run = [a for n, a in dyn_calls(before) if n == "rcfm_busdyn_run"][0]
    mixrun = [a for n, a in fake.calls[before:] if n == "rcfm_mix_run"][0]
    assert run[1] == A and run[2] == mixrun[7] and run[3] == mixrun[9]            # the mixer's out and bus_open
    wet, active, open_out = t._last.mix[1][0]
    dry, active2, bus_open, L = t._last.dry[1][0]
    assert run[4:6] == (wet.data_ptr(), open_out.data_ptr()) and wet.shape == dry.shape == (2, A, 2) and active is active2
    assert (dry.data_ptr(), bus_open.data_ptr()) == (mixrun[7], mixrun[9]) and L == 64
    assert t.mix() is wet and t.mix(dry=True) is dry and t.bus_delay() == [64]
    # the next run uses the same handle
    t.load(x)
    t.run_all()
    assert fake.count("rcfm_busdyn_create") == 1 and fake.count("rcfm_busdyn_run") == 2
    # without ducks the four tables are NULL
    t.set_bus_dynamics(rc.Limiter(lookahead=0.002))
    t.run_all()
    assert fake.count("rcfm_busdyn_create") == 2
    create = [a for n, a in dyn_calls() if n == "rcfm_busdyn_create"][-1]
    assert create[2] == 16 and create[6:10] == (None, None, None, None)
    # run_all_packed(buses=True): the pack reads the processed rows and bus_open_out
    drain = rc.Drain(2, (A, 2), "int16", depth=2)
    before = len(fake.calls)
    assert t.run_all_packed(rc.PCM("int16"), drain=drain, buses=True) is None
    pack = [a for n, a in fake.calls[before:] if n == "rcfm_audio_pack"][0]
    wet, _, open_out = t._last.mix[1][0]
    assert pack[0] == wet.data_ptr() and pack[1] == open_out.data_ptr() and pack[2] == 2 and pack[3] == 2 * A
    assert [n for n, _ in fake.calls[before:]][-4:] == ["rcfm_mix_run", "rcfm_busdyn_run", "rcfm_audio_pack", "rcfm_drain_submit"]
    # a growing channel list: a new mixer handle, the same dynamics handle (the audio length stays)
    t.add_channel(446.0e6 + float(B) * C, B, rc.FM(B, A))
    t.request_bandwidth(float(N))
    t.load(x)
    t.run_all()
    assert fake.count("rcfm_busdyn_create") == 2 and fake.count("rcfm_mix_create") == 2
    # reset_states resets the handle
    t.reset_states()
    assert fake.count("rcfm_busdyn_reset") == 1
    # lanes share the setting and the handles, behind a fence
    t._arm_state_fence()
    assert fake.count("rcfm_busdyn_set_fence") == 1
    lane = t._lane_clone()
    assert lane._busdyn is t._busdyn and lane._busdyn_handles is t._busdyn_handles
    lane.load(x)
    lane.run_all()
    assert fake.count("rcfm_busdyn_create") == 2
    t.set_bus_dynamics(rc.Limiter())
    assert not t._busdyn_handles
    lane._sync_lane(t)
    lane.run_all()
    t.run_all()
    assert fake.count("rcfm_busdyn_create") == 3 and fake.count("rcfm_busdyn_set_fence") == 2      # made by the lane, fenced, used by both
    # off again: nothing more of it, the call trace of a tuner that never had it
    t.set_bus_dynamics()
    assert t._busdyn is None and not t._busdyn_handles
    before = len(fake.calls)
    t.load(x)
    t.run_all()
    assert not [n for n, _ in dyn_calls(before) if n != "rcfm_busdyn_destroy"]
    never = tuner(channels=C + 1)
    never.set_mix(mixer)
    never.set_squelch(1e-3)
    never.load(x)
    mark = len(fake.calls)
    never.run_all()
    assert [n for n, _ in fake.calls[before:mark] if n in ("rcfm_pipeline_run", "rcfm_tuner_levels", "rcfm_squelch", "rcfm_mix_run")] == \
        [n for n, _ in fake.calls[mark:] if n in ("rcfm_pipeline_run", "rcfm_tuner_levels", "rcfm_squelch", "rcfm_mix_run")]
    assert t.mix(dry=True) is t.mix() and t.bus_delay() == [0]
    # set_mix(None) takes the dynamics along; another mixer restarts them; its ducks must resolve
    t.set_bus_dynamics(rc.Limiter(), ducks={"rest": rc.Duck("tower")})
    t.run_all()
    assert t._busdyn_handles
    with pytest.raises(ValueError):
        t.set_mix(rc.Mixer([tower]))                       # no bus "rest"
    assert t._mix is mixer and t._busdyn_handles
    t.set_mix(rc.Mixer([rest, tower]))
    assert not t._busdyn_handles and t._busdyn is not None
    t.set_mix(None)
    assert t._busdyn is None
    # reset() drops the handles
    t.set_mix(mixer)
    t.set_bus_dynamics(rc.Limiter())
    t.run_all()
    assert t._busdyn_handles
    with pytest.raises(ValueError):
        t.reset()
    assert not t._busdyn_handles
    # run_each: one handle per group at the group's rate; a duck across two groups is refused before anything is launched
    e = tuner(channels=4, wide=2)
    e.set_mix(rc.Mixer([rc.Bus.of([0, 1, 3]), rc.Bus.of([5, 4]), rc.Bus.of([2])]))
    e.set_bus_dynamics(rc.Limiter(), ducks={2: rc.Duck(0)})
    e.load(x)
    before = len(fake.calls)
    e.run_each()
    assert [n for n, _ in dyn_calls(before)].count("rcfm_busdyn_create") == 2
    runs = [a for n, a in dyn_calls(before) if n == "rcfm_busdyn_run"]
    assert len(runs) == 2 and runs[0][0] != runs[1][0] and e.bus_delay() == [64, 64] and len(e.mix()) == 3 and len(e.mix(dry=True)) == 3
    names = [n for n, _ in fake.calls[before:] if n in ("rcfm_mix_run", "rcfm_busdyn_run")]
    assert names == ["rcfm_mix_run", "rcfm_busdyn_run"] * 2
    e.set_bus_dynamics(rc.Limiter(), ducks={1: rc.Duck(0)})
    before = len(fake.calls)
    with pytest.raises(ValueError, match="launch group"):
        e.run_each()
    assert not [n for n, _ in fake.calls[before:] if n in ("rcfm_pipeline_run", "rcfm_mix_run", "rcfm_busdyn_run")]
    # under shard and with a window attached: refused, as set_mix is
    late = tuner()
    late.set_mix(mixer)
    late.set_bus_dynamics(rc.Limiter())
    late.shard(0, 3)
    late.load(x)
    before = len(fake.calls)
    with pytest.raises(RuntimeError):
        late.run_all()
    assert not [n for n, _ in fake.calls[before:] if n in ("rcfm_pipeline_run", "rcfm_busdyn_run")]
    with pytest.raises(ValueError):
        late.set_bus_dynamics(rc.Limiter())
    attached = tuner()
    attached.set_mix(mixer)
    attached._slot = object()
    with pytest.raises(ValueError):
        attached.set_bus_dynamics(rc.Limiter())
