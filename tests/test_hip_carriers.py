"""GPU: per-channel carrier estimates (rcfm_tuner_carriers) and live retune (rcfm_tuner_retune) against their definition
in include/rcfm.h, evaluated by tests/carrier_model.py in float64 on the same complex64 input.

Bounds: peak_bin exact (tests/test_carriers.py proves on the CPU that every channel's strongest bin leads by >= 6 dB and
that no bin lies within 1e-3 of the gate); peak_power within 3e-5 relative (the bound of tests/test_hip_spectrum.py for
the same quantity); centroid and spread absolute in bins, within 4 x the pinned float32 CPU figure of the case
(carrier_model.YARDSTICK).  Every case prints its worst channel.  Retune: bit-identical to a Tuner built with the shifted
channel frequencies -- the same tables drive the same kernels.
"""

import ctypes

import numpy as np
import pytest

import carrier_model as cm
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ERR_INDEX, ERR_ARG, ERR_STATE = -2, -4, -5


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def hip(rc):
    from radiocore._internal import hip
    return hip


def _create(hip, n, rolls, bws):
    h = ctypes.c_void_p()
    hip.check(hip.lib().rcfm_tuner_create(n, len(rolls), (ctypes.c_int64 * len(rolls))(*rolls),
                                          (ctypes.c_int32 * len(bws))(*bws), ctypes.byref(h)))
    return hip.Handle(h, hip.lib().rcfm_tuner_destroy)


def _raw(hip, h, first, count, gate, which=(True, True, True, True), stream=None):
    """rcfm_tuner_carriers into fresh tensors (None where `which` is False); returns (status, host arrays)."""
    import torch
    dts = (torch.int32, torch.float32, torch.float32, torch.float32)
    out = [torch.full((max(count, 1),), -7, dtype=dt, device="cuda") if w else None for dt, w in zip(dts, which)]
    rc_ = hip.lib().rcfm_tuner_carriers(h.value, first, count, ctypes.c_float(gate), *[hip.ptr(o) if o is not None else None for o in out],
                                        stream if stream is not None else hip.stream())
    torch.cuda.synchronize()
    return rc_, [o.cpu().numpy()[:count] if o is not None else None for o in out]


def _check(got, exp, bounds, what):
    pb, pp, ce, sp = got
    assert pb.dtype == np.int32 and pp.dtype == ce.dtype == sp.dtype == np.float32
    rel = np.abs(pp - exp[1]) / exp[1]
    dc, ds = np.abs(ce - exp[2]), np.abs(sp - exp[3])
    print("%s: %d channels, peak_bin mismatches %d, peak_power %.3g relative (channel %d), centroid %.3g bins (channel %d, "
          "bound %.3g), spread %.3g bins (channel %d, bound %.3g)"
          % (what, pb.size, int(np.sum(pb != exp[0])), rel.max(), rel.argmax(), dc.max(), dc.argmax(), bounds[0], ds.max(),
             ds.argmax(), bounds[1]))
    assert np.array_equal(pb, exp[0]), (what, np.flatnonzero(pb != exp[0]))
    assert rel.max() <= cm.PEAK_POWER_REL, (what, rel.max())
    assert dc.max() <= bounds[0], (what, dc.max(), bounds[0])
    assert ds.max() <= bounds[1], (what, ds.max(), bounds[1])


def _loaded(hip, name):
    import torch
    n, rolls, bws, x, _ = cm.case(name)
    h = _create(hip, n, rolls, bws)
    xd = hip.to_device(x.copy())                 # (the shared case stays read-only)
    hip.check(hip.lib().rcfm_tuner_load(h.value, hip.ptr(xd), hip.stream()))
    torch.cuda.synchronize()
    halo, nn = ctypes.c_int64(), ctypes.c_int64()
    hip.check(hip.lib().rcfm_tuner_spectrum_layout(h.value, ctypes.byref(halo), ctypes.byref(nn)))
    return h, len(rolls), int(halo.value)


# ---- the kernels against the model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fast", "odd900001", "odd90001", "general"])
def test_carriers_against_the_model(hip, name):
    """fast: N = 4 000 000, one handle mixing B = 25 000 / 12 500 / 2001 / 7, both base parities, tones at the first and
    last bin and on both sides of every segment boundary, runs that start and end in the halos, the band edges.
    odd*: odd N and odd B.  general: a channel with B = n leaves the handle without halos -- 64-bit modulo indexing.
    Each with gate 0 and with a gate between the noise and the sidebands; twice bit-identical; a sub-range of mixed
    bandwidths equals the same channels of the whole range."""
    h, C, halo = _loaded(hip, name)
    assert (halo == 0) == (name == "general")
    for gate in cm.GATES:
        st, got = _raw(hip, h, 0, C, gate)
        assert st == 0
        _check(got, cm.expected(name, gate), cm.gpu_bounds(name, gate), "%s gate %g" % (name, gate))
        st, again = _raw(hip, h, 0, C, gate)
        assert st == 0 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again))
        first, count = C // 3, C - C // 3 - 1
        st, part = _raw(hip, h, first, count, gate)
        assert st == 0 and all(np.array_equal(a[first:first + count].view(np.uint32), b.view(np.uint32)) for a, b in zip(got, part))


def test_determinism_streams_and_null_outputs(hip):
    """Bit-identical on a second stream and with each single output alone against all four together; the untouched
    tensors of a NULL output are not written."""
    import torch
    h, C, _ = _loaded(hip, "fast")
    _, ref = _raw(hip, h, 0, C, cm.GATE)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st, got = _raw(hip, h, 0, C, cm.GATE, stream=ctypes.c_void_p(side.cuda_stream))
    assert st == 0 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ref, got))
    for k in range(4):
        which = tuple(i == k for i in range(4))
        st, got = _raw(hip, h, 0, C, cm.GATE, which=which)
        assert st == 0 and np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
        assert all(got[i] is None for i in range(4) if i != k)


def test_argument_and_state_errors(hip):
    import torch
    lib = hip.lib()
    n, rolls, bws, x, _ = cm.case("odd90001")
    h = _create(hip, n, rolls, bws)
    out = torch.empty(4, dtype=torch.float32, device="cuda")
    p, s = hip.ptr(out), hip.stream()
    f = ctypes.c_float
    assert lib.rcfm_tuner_carriers(None, 0, 1, f(0.0), p, p, p, p, s) == ERR_ARG
    assert lib.rcfm_tuner_carriers(h.value, 0, 1, f(0.0), None, None, None, None, s) == ERR_ARG
    for bad in (-1e-9, float("nan"), float("inf")):
        assert lib.rcfm_tuner_carriers(h.value, 0, 1, f(bad), p, None, None, None, s) == ERR_ARG
    assert lib.rcfm_tuner_carriers(h.value, 0, 2, f(0.0), None, p, None, None, s) == ERR_STATE          # before a load
    xd = hip.to_device(x.copy())
    hip.check(lib.rcfm_tuner_load(h.value, hip.ptr(xd), s))
    assert lib.rcfm_tuner_carriers(h.value, 0, 3, f(0.0), None, p, None, None, s) == ERR_INDEX
    assert lib.rcfm_tuner_carriers(h.value, -1, 1, f(0.0), None, p, None, None, s) == ERR_INDEX
    hip.check(lib.rcfm_tuner_carriers(h.value, 1, 0, f(0.0), None, p, None, None, s))                   # an empty range
    assert lib.rcfm_tuner_retune(None, 0, 0, None, s) == ERR_ARG
    assert lib.rcfm_tuner_retune(h.value, 0, 1, None, s) == ERR_ARG
    assert lib.rcfm_tuner_retune(h.value, 1, 2, (ctypes.c_int64 * 2)(0, 0), s) == ERR_INDEX
    hip.check(lib.rcfm_tuner_retune(h.value, 2, 0, None, s))
    torch.cuda.synchronize()


# ---- through the Python Tuner: readiness, retune ---------------------------------------------------------------------------

N, B, C, A = cm.GRID_N, cm.GRID_B, cm.GRID_C, 8000
OFFSETS = cm.GRID_OFFSETS


def _grid(rc, kind="AM", shift=None):
    """A Tuner over carrier_model.case_grid's channels (every f_in - f_c a whole number); shift[c] moves the centres."""
    t = rc.Tuner()
    for i in range(C):
        f = 100e6 + float(cm.GRID_RASTER) * (i - C // 2) + (float(shift[i]) if shift is not None else 0.0)
        t.add_channel(f, B, getattr(rc, kind)(B, A) if kind else None)
    t.request_bandwidth(float(N))
    return t


def _band(t, seed=3):
    """carrier_model.case_grid's buffer: one modulated tone per channel, OFFSETS[c] bins off its centre."""
    n, rolls, _, x, _ = cm.case("grid")
    assert rolls == [int(t.input_frequency - c.center_frequency) for c in t.channels()] and n == N
    return rolls, x.copy() if seed == 3 else cm.case_grid(seed)[2]


def test_tuner_carriers_shard_window_and_slot(rc, hip):
    """Tuner.carriers on the handle's own spectrum against the model; after shard, through an attached window + adopt and
    on an attached slot: the same bits.  RCFM_ERR_STATE outside the window."""
    lib = hip.lib()
    t = _grid(rc)
    rolls, x = _band(t)
    t.load(x)
    for gate in cm.GATES:
        got = t.carriers(gate)
        assert np.array_equal(got[0], OFFSETS)
        _check(got, cm.expected("grid", gate), cm.gpu_bounds("grid", gate), "tuner gate %g" % gate)
    whole = t.carriers(cm.GATE)
    first, count = 14, 8               # clear of the band centre: their bins do not wrap around bin 0
    sh = _grid(rc)
    sh.shard(first, count)
    sh.load(x)
    assert all(np.array_equal(a, b[first:first + count]) for a, b in zip(sh.carriers(cm.GATE), whole))
    win = _grid(rc)
    win.shard(first, count)
    slot = win.window_slot(N, first, count)
    assert slot is not None
    fb, nb = win.window(N, first, count)
    win.attach_window(slot, N)
    Xp = ctypes.c_void_p()
    hip.check(lib.rcfm_tuner_spectrum(t._handle.value, ctypes.byref(Xp)))
    hip.check(lib.rcfm_memcpy_d2d(ctypes.c_void_p(slot.data_ptr() + 8 * slot.rcfm_halo), ctypes.c_void_p(Xp.value + 8 * fb),
                                  ctypes.c_size_t(8 * nb), hip.stream()))
    win.adopt(N, first, count)
    assert all(np.array_equal(a, b[first:first + count]) for a, b in zip(win.carriers(cm.GATE), whole))
    import torch
    out = torch.empty(C, dtype=torch.float32, device="cuda")
    assert lib.rcfm_tuner_carriers(win._handle.value, first - 1, 2, ctypes.c_float(0.0), None, hip.ptr(out), None, None,
                                   hip.stream()) == ERR_STATE
    with pytest.raises(RuntimeError):                                   # refused while a window is attached
        win.retune(1)
    assert win.fine_tune().tolist() == [0] * C
    att = _grid(rc)
    att.attach(att.spectrum_slot(N), N)
    att.load(x)
    assert all(np.array_equal(a, b) for a, b in zip(att.carriers(cm.GATE), whole))


@pytest.mark.parametrize("kind", ["AM", "USB", "FM"])
def test_retune_equals_a_tuner_built_there(rc, hip, kind):
    """After retune(peak_bin): run(c) and run_all are bit-identical to a fresh Tuner with the shifted channel
    frequencies on the same buffer, carriers reads peak_bin - k, and levels follow; the buffer is not loaded again."""
    t = _grid(rc, kind)
    _, x = _band(t)
    t.load(x)
    pb, pp, ce, _ = t.carriers()
    assert pb.tolist() == OFFSETS
    before = t.levels()
    k = rc.tools.afc.corrections(pb, pp, ce, 1e-4, 5000)
    assert k.tolist() == OFFSETS
    handle = t._handle
    t.retune(k)
    assert t._handle is handle and t.fine_tune().tolist() == OFFSETS
    fresh = _grid(rc, kind, shift=OFFSETS)
    assert fresh.input_frequency == t.input_frequency and list(fresh._rolls(None)) == list(t._rolls(t._fine))
    fresh.load(x)
    assert not t.carriers()[0].any()
    assert np.array_equal(t.levels(), fresh.levels()) and not np.array_equal(t.levels(), before)
    for c in (0, 1, 9, C - 1):
        assert np.array_equal(t.run(c), fresh.run(c)), c
    assert np.array_equal(t.run_all(), fresh.run_all())
    thr = rc.tools.threshold_over_floor(fresh.levels(), B, 3.0)
    t.set_squelch(thr)
    fresh.set_squelch(thr)
    assert np.array_equal(t.run_all(), fresh.run_all()) and np.array_equal(t.open_mask(), fresh.open_mask())
    t.retune(-2)                                                        # cumulative
    assert t.carriers()[0].tolist() == [2] * C
    lane = t._lane_clone()                                              # a handle created later starts from the retuned rolls
    lane.load(x)
    assert lane._handle is not handle and lane.carriers()[0].tolist() == [2] * C


def test_retune_range_leaves_the_other_channels(rc, hip):
    """rcfm_tuner_retune(first = 3, count = 2): channels 3 and 4 read as a Tuner built there, every other channel is
    bit-identical to before."""
    t = _grid(rc, None)
    _, x = _band(t)
    t.load(x)
    before = [t.run(c) for c in range(C)]
    rolls = list(t._rolls(None))
    new = (ctypes.c_int64 * 2)(rolls[3] - OFFSETS[3] + 5 * N, rolls[4] - OFFSETS[4] - 2 * N)      # reduced modulo n
    hip.check(hip.lib().rcfm_tuner_retune(t._handle.value, 3, 2, new, hip.stream()))
    new[0] = new[1] = 0                                                 # the values were staged
    fresh = _grid(rc, None, shift=[OFFSETS[i] if i in (3, 4) else 0 for i in range(C)])
    fresh.load(x)
    for c in range(C):
        got = t.run(c)
        assert np.array_equal(got, fresh.run(c)), c
        assert np.array_equal(got, before[c]) == (c not in (3, 4)), c
    assert t.carriers()[0].tolist() == [0 if i in (3, 4) else OFFSETS[i] for i in range(C)]


def test_retune_after_a_sharded_load_needs_a_reload(rc, hip):
    sh = _grid(rc)
    _, x = _band(sh)
    first, count = 14, 8
    sh.shard(first, count)
    sh.load(x)
    assert sh.carriers()[0].tolist() == OFFSETS[first:first + count]
    fb, nb = sh.window(N, first, count)
    sh.retune(OFFSETS)
    if nb < N:                                                          # the storage held a window for the old rolls
        with pytest.raises(RuntimeError):
            sh.carriers()
        with pytest.raises(RuntimeError):
            sh.run_all()
    sh.load(x)
    assert not sh.carriers()[0].any()
    fresh = _grid(rc, shift=OFFSETS)
    fresh.shard(first, count)
    fresh.load(x)
    assert np.array_equal(sh.run_all(), fresh.run_all())


def test_lanes_follow_the_retune(rc, hip):
    """Lanes(depth=2) over a retuned tuner, and over a tuner retuned between submissions: the audio of plain run_all."""
    from radiocore.tools import Lanes
    base = _grid(rc)
    _, x0 = _band(base, seed=3)
    _, x1 = _band(base, seed=4)
    fresh = _grid(rc, shift=OFFSETS)
    want = []
    for x in (x0, x1, x0):
        fresh.load(x)
        want.append(fresh.run_all())
    plain = _grid(rc)
    plain.load(x0)
    unshifted = plain.run_all()
    lanes = Lanes(base, depth=2)
    a = lanes.result(lanes.submit(x0))
    b = lanes.result(lanes.submit(x0))
    assert np.array_equal(a, unshifted) and np.array_equal(b, unshifted)
    base.retune(OFFSETS)
    tickets = [lanes.submit(x) for x in (x0, x1, x0)]
    for i, tk in enumerate(tickets):
        assert np.array_equal(lanes.result(tk), want[i]), i


def test_airband_afc_example():
    """examples/airband_afc.py at a reduced size: the measured offsets are the planted ones and the second pass reads 0."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("airband_afc", os.path.join(ROOT, "examples", "airband_afc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    on_air, truth, measured, after = mod.run(channels=120, rate=4_000_000, stations=12)
    assert len(on_air) == 12 and any(truth)
    assert [int(v) for v in measured] == [int(v) for v in truth]
    assert not any(after)
