"""GPU: the noise floor (include/rcfm.h, "noise floor") against tests/floor_model.py.

rcfm_rank_filter, rcfm_floor_run, rcfm_floor_thresholds: output bits equal the model's -- the selection is exact and the
smoothing is three float32 roundings in a stated order, so there is no tolerance.
Through the Tuner: the floor equals the model applied to the device's own power spectrum bit for bit, and lies within
6e-6 relative (REL_64["power"] of tests/test_hip_spectrum.py, which the monotone, scale-equivariant filter carries through
unchanged: tests/test_floor_model.py) plus 2 float32 ulps per smoothing step of the float64 truth; masks equal the model's on
the scene whose levels tests/test_floor_model.py proves to lie >= 3 dB from every threshold.
"""

import ctypes

import numpy as np
import pytest

import floor_model as fm
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

REL_POWER = 6e-6                  # tests/test_hip_spectrum.py, REL_64["power"]
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def hip(rc):
    from radiocore._internal import hip
    return hip


@pytest.fixture(scope="module")
def torch(rc):
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(torch, a, offset_floats=0):
    """The array on the device, its first element `offset_floats` floats behind an allocation's start."""
    a = np.ascontiguousarray(a)
    flat = torch.from_numpy(a.view(np.uint8).reshape(-1))
    buf = torch.empty(flat.numel() + 4 * offset_floats + 64, dtype=torch.uint8, device="cuda")
    view = buf[4 * offset_floats:4 * offset_floats + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 256 == (4 * offset_floats) % 256
    return view


def _rank_filter(hip, torch, xd, M, half, guard, q, stream=None, offset_floats=0):
    buf = torch.full((M + 2 + offset_floats,), -1.0, dtype=torch.float32, device="cuda")
    out = buf[offset_floats:]
    hip.check(hip.lib().rcfm_rank_filter(ctypes.c_void_p(xd.data_ptr()), M, half, guard, q, hip.ptr(out),
                                         hip.stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)))
    if stream is not None:
        stream.synchronize()
    got = out.cpu().numpy()
    assert got[M] == -1.0 and got[M + 1] == -1.0             # nothing behind the last cell was written
    return got[:M]


def _inputs(M, seed):
    """name -> float32 [M]: tilted exponential noise; four levels (heavy in ties); a constant; the four levels with +-0,
    denormals, +-inf and NaNs of both signs sprinkled in; NaN throughout but for a few cells (whole windows of NaN)."""
    rng = np.random.default_rng(seed)
    tilt = 10.0 ** (2.0 * np.arange(M) / M)
    levels = rng.choice(np.array([0.5, 1.0, 2.0, 4.0], np.float32), size=M)
    awkward = levels.copy()
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan, -np.nan, -3.0], np.float32)
    hit = rng.random(M) < 0.3
    awkward[hit] = rng.choice(special, size=int(hit.sum()))
    nans = np.full(M, np.nan, np.float32)
    nans[::max(M // 3, 1)] = 1.5
    return {"tilted": (rng.exponential(1.0, M) * tilt).astype(np.float32), "levels": levels, "constant": np.full(M, 3.0, np.float32),
            "awkward": awkward, "nans": nans}


# (M, half, guard, q): M in {guard + 2, 3, 255, 256, 257, 1000, 70 001}, half in {1, 2, 7, 63, 64, 65, 300} and 4096 at
# M = 10 000, guard in {0, 1, half - 1}, q in {0, 1, 250, 500, 999, 1000} -- a subset in which every value of each occurs with
# several of the others.  256 cells are a workgroup's: 255 / 256 / 257 and 1000 end inside one, 70 001 has 274; half = 300
# and 4096 reach over more than one workgroup; M <= half cuts every window at both ends.
SHAPES = [(2, 1, 0, 500), (3, 2, 1, 250), (8, 7, 6, 0), (64, 63, 62, 1000), (66, 65, 64, 1), (301, 300, 299, 500),
          (3, 1, 0, 0), (3, 2, 0, 999), (3, 7, 1, 500), (3, 64, 0, 1000),
          (255, 1, 0, 1), (255, 7, 1, 250), (255, 63, 62, 500), (255, 300, 0, 1000),
          (256, 2, 1, 0), (256, 64, 0, 250), (256, 65, 64, 999), (256, 300, 1, 500),
          (257, 1, 0, 1000), (257, 7, 6, 1), (257, 64, 1, 500), (257, 300, 0, 250), (257, 2, 0, 999),
          (1000, 2, 0, 250), (1000, 7, 0, 999), (1000, 63, 1, 0), (1000, 64, 63, 500), (1000, 65, 0, 1), (1000, 300, 1, 250),
          (1000, 300, 0, 1000), (1000, 63, 62, 250),
          (70001, 1, 0, 500), (70001, 7, 1, 250), (70001, 63, 0, 0), (70001, 64, 1, 1000), (70001, 65, 64, 999),
          (70001, 300, 1, 250), (70001, 2, 1, 1),
          (10000, 4096, 0, 250), (10000, 4096, 4095, 500), (10000, 4096, 1, 999)]


@pytest.mark.parametrize("M,half,guard,q", SHAPES)
def test_rank_filter_against_model(hip, torch, M, half, guard, q):
    for name, x in _inputs(M, 1000 * half + guard + q).items():
        got = _rank_filter(hip, torch, _dev(torch, x), M, half, guard, q)
        want = fm.rank_filter(x, half, guard, q)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, (name, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("M,half,guard,q", [(1000, 64, 1, 250), (70001, 65, 0, 500), (257, 300, 1, 999)])
def test_rank_filter_bit_identity(hip, torch, M, half, guard, q):
    """Two runs; a second stream; x and out on a base that is 4 but not 16 bytes aligned."""
    x = _inputs(M, M)["awkward"]
    xd = _dev(torch, x)
    first = _rank_filter(hip, torch, xd, M, half, guard, q)
    assert np.array_equal(_bits(first), _bits(_rank_filter(hip, torch, xd, M, half, guard, q)))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(first), _bits(_rank_filter(hip, torch, xd, M, half, guard, q, stream=torch.cuda.Stream())))
    shifted = _dev(torch, x, offset_floats=1)
    assert shifted.data_ptr() % 16 == 4
    for off in (0, 3):
        assert np.array_equal(_bits(first), _bits(_rank_filter(hip, torch, shifted, M, half, guard, q, offset_floats=off)))


# ---- the handle ----------------------------------------------------------------------------------------------------------

class _Floor:
    def __init__(self, hip, M, half, guard, q, rise, fall):
        self.hip, self.lib, self.M = hip, hip.lib(), M
        h = ctypes.c_void_p()
        hip.check(self.lib.rcfm_floor_create(M, half, guard, q, rise, fall, ctypes.byref(h)))
        self.handle = hip.Handle(h, self.lib.rcfm_floor_destroy)

    def run(self, torch, power, ratio, want_floor=True, want_over=True):
        pd = _dev(torch, np.ascontiguousarray(power, dtype=np.float32))
        floor = torch.full((self.M + 1,), -1.0, dtype=torch.float32, device="cuda")
        over = torch.full((self.M + 1,), 7, dtype=torch.uint8, device="cuda")
        self.hip.check(self.lib.rcfm_floor_run(self.handle.value, ctypes.c_void_p(pd.data_ptr()), ratio,
                                               self.hip.ptr(floor) if want_floor else None,
                                               self.hip.ptr(over) if want_over else None, self.hip.stream()))
        f, o = floor.cpu().numpy(), over.cpu().numpy()
        assert f[-1] == -1.0 and o[-1] == 7
        assert want_floor or np.all(f == -1.0)
        assert want_over or np.all(o == 7)
        return f[:-1], o[:-1]

    def state(self):
        s = np.zeros(self.M, np.float32)
        self.hip.check(self.lib.rcfm_floor_get_state(self.handle.value, s.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), self.hip.stream()))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, dtype=np.float32)
        self.hip.check(self.lib.rcfm_floor_set_state(self.handle.value, s.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), self.hip.stream()))


def test_floor_run_against_model(hip, torch):
    """Three calls with the state carried -- unprimed, the rise branch, the fall branch -- each output NULL in turn; a NaN
    estimate leaves the state; `over` at values equal to ratio s'; reset; the get / set_state round trip."""
    rng = np.random.default_rng(21)
    M, half, guard, q = 1000, 40, 5, 250
    rise, fall = np.float32(fm.factor(10.0)), np.float32(fm.factor(1.0))
    f = _Floor(hip, M, half, guard, q, float(rise), float(fall))
    assert np.all(_bits(f.state()) == 0x7fc00000)                       # not primed
    p1 = (rng.exponential(1.0, M) * 10.0 ** (2.0 * np.arange(M) / M)).astype(np.float32)
    powers = [p1, (4.0 * p1 * rng.uniform(0.9, 1.1, M)).astype(np.float32), (0.25 * p1 * rng.uniform(0.9, 1.1, M)).astype(np.float32)]
    s = np.full(M, np.nan, np.float32)
    for k, (p, outputs) in enumerate(zip(powers, ((True, True), (True, False), (False, True)))):
        prev = s
        s, over = fm.floor_run(s, p, half, guard, q, rise, fall, 4.0)
        got_floor, got_over = f.run(torch, p, 4.0, *outputs)
        if outputs[0]:
            assert np.array_equal(_bits(got_floor), _bits(s)), k
        if outputs[1]:
            assert np.array_equal(got_over, over) and 0 < int(over.sum()) < M, k
        assert np.array_equal(_bits(f.state()), _bits(s)), k
        if k == 1:
            assert np.all(s > prev)                                      # the slow factor upwards ...
        if k == 2:
            assert np.all(s < prev)                                      # ... the fast one downwards
    # windows of NaN: those cells keep their state, the others move
    holed = powers[0].copy()
    holed[300:500] = np.nan
    want, over = fm.floor_run(s, holed, half, guard, q, rise, fall, 4.0)
    assert np.array_equal(_bits(want[345:455]), _bits(s[345:455])) and not np.array_equal(want[:300], s[:300])
    got_floor, got_over = f.run(torch, holed, 4.0)
    assert np.array_equal(_bits(got_floor), _bits(want)) and np.array_equal(got_over, over) and not got_over[300:500].any()
    # reset: not primed again; equality is over, one float32 step below is not
    hip.check(hip.lib().rcfm_floor_reset(f.handle.value, hip.stream()))
    assert np.all(_bits(f.state()) == 0x7fc00000)
    ratio = np.float32(2.5118864)
    flat = np.full(M, 3.0, np.float32)
    edge = np.float32(ratio * np.float32(3.0))                          # (one float32 product, as the kernel's)
    flat[100], flat[200], flat[300] = edge, np.nextafter(edge, np.float32(0.0)), np.nextafter(edge, np.float32(np.inf))
    want, over = fm.floor_run(np.full(M, np.nan, np.float32), flat, half, guard, q, rise, fall, ratio)
    assert np.all(want == 3.0) and over[100] == 1 and over[200] == 0 and over[300] == 1 and int(over.sum()) == 2
    got_floor, got_over = f.run(torch, flat, float(ratio))
    assert np.array_equal(_bits(got_floor), _bits(want)) and np.array_equal(got_over, over)
    # state round trip: NaN, -0 and denormals come back as they went
    odd = rng.exponential(1.0, M).astype(np.float32)
    odd[:4] = [np.nan, -0.0, 1e-45, np.inf]
    f.set_state(odd)
    assert np.array_equal(_bits(f.state()), _bits(odd))
    want, _ = fm.floor_run(odd, powers[0], half, guard, q, rise, fall, 1.0)
    got_floor, _ = f.run(torch, powers[0], 1.0)
    assert np.array_equal(_bits(got_floor[1:]), _bits(want[1:])) and np.array_equal(_bits(got_floor[:1]), _bits(want[:1]))


def test_floor_thresholds_against_model(hip, torch):
    rng = np.random.default_rng(3)
    M, count = 400, 777
    floor = rng.exponential(1.0, M).astype(np.float32)
    floor[7] = np.nan
    cell = rng.integers(0, M, count).astype(np.int32)
    cell[:8] = [-1, M, M + 1000, -2 ** 31, 2 ** 31 - 1, 0, M - 1, 7]
    gain = rng.uniform(0.01, 30.0, count).astype(np.float32)
    out = torch.full((count + 1,), -1.0, dtype=torch.float32, device="cuda")
    fd, cd, gd = _dev(torch, floor), _dev(torch, cell), _dev(torch, gain)      # (held: three allocations, not one reused)
    hip.check(hip.lib().rcfm_floor_thresholds(ctypes.c_void_p(fd.data_ptr()), M, ctypes.c_void_p(cd.data_ptr()),
                                              ctypes.c_void_p(gd.data_ptr()), count, hip.ptr(out), hip.stream()))
    got = out.cpu().numpy()
    want = fm.thresholds(floor, cell, gain)
    assert got[-1] == -1.0 and np.isnan(want[:5]).all() and np.isnan(want[7]) and not np.isnan(want[5:7]).any()
    assert np.array_equal(np.isnan(want[8:]), cell[8:] == 7) and not np.isnan(want[8:]).all()
    assert np.array_equal(np.isnan(got[:-1]), np.isnan(want)) and np.array_equal(_bits(got[:-1])[~np.isnan(want)], _bits(want)[~np.isnan(want)])
    assert np.all(_bits(got[:5]) == 0x7fc00000)


# ---- through the Tuner ---------------------------------------------------------------------------------------------------

DROP = 10.0 ** -0.6                   # the noise 6 dB down
SCALES = (1.0, DROP, DROP)


@pytest.fixture(scope="module")
def buffers():
    return [fm.buffer(1 + b, scale=s) for b, s in enumerate(SCALES)]


def _demod(rc, kind):
    return lambda: getattr(rc, kind)(fm.B, fm.A)


def _tuner(rc, kind="FM", floor=True, channels=None):
    t = rc.Tuner()
    cs = fm.centres()
    for i in (range(fm.C) if channels is None else channels):
        t.add_channel(cs[i], fm.B, _demod(rc, kind)())
    t.request_bandwidth(float(fm.N))
    if floor:
        t.set_floor(_nf(rc))
    return t


def _nf(rc):
    return rc.NoiseFloor(fm.CELL_HZ, half=fm.HALF, guard=fm.GUARD, quantile=fm.QUANTILE)


def _factors(rc):
    return _nf(rc).factors


STATIONS = np.isin(np.arange(fm.C), list(fm.STATIONS))


def test_tuner_floor_against_model_and_truth(rc, buffers):
    """floor() of three buffers: the model on the device's own power spectrum, bit for bit; the float64 truth within 6e-6 plus
    2 float32 ulps per smoothing step; floor_levels() and occupied_cells() from the same floor."""
    t = _tuner(rc)
    rise, fall = _factors(rc)
    s = np.full(fm.CELLS, np.nan, np.float32)
    s64 = np.full(fm.CELLS, np.nan)
    for b, x in enumerate(buffers):
        t.load(x)
        p = t.power_spectrum(fm.CELLS)
        s, _ = fm.floor_run(s, p, fm.HALF, fm.GUARD, 250, rise, fall, 1.0)
        got = t.floor()
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(s)), b
        s64 = fm.smooth(s64, fm.rank_filter64(fm.cell_power64(x), fm.HALF, fm.GUARD, 250), float(rise), float(fall), dtype=np.float64)
        rel = float(np.max(np.abs(got / s64 - 1.0)))
        print("buffer %d: floor against float64 truth, worst relative error %.3g" % (b, rel))
        assert rel <= REL_POWER + 2.0 * b * ULP, (b, rel)
        assert np.array_equal(_bits(t.floor_levels()), _bits(fm.thresholds(s, fm.channel_cells(), fm.gains(0.0))))
        want = p >= (np.float32(10.0 ** 0.8) * s).astype(np.float32)
        assert np.array_equal(t.occupied_cells(8.0), want)
        # the stations' own cells are occupied, and next to nothing else
        cells = fm.channel_cells()
        assert want[cells[STATIONS]].all() and int(want.sum()) <= 3 * 7 + 4
    # the floor followed the drop by `fall`: 1 - (1 - a)^2 of the way after two buffers
    drop = np.median(s / fm.rank_filter(t.power_spectrum(fm.CELLS), fm.HALF, fm.GUARD, 250))
    assert 1.0 < drop < 1.0 + 3.0 * (1.0 - float(fall)) ** 2 * 1.3


@pytest.mark.parametrize("kind", ["AM", "FM"])
def test_tuner_squelch_over_floor(rc, buffers, kind):
    """set_squelch(OverFloor(8)): the masks are the model's -- stations open, empty channels closed -- where no fixed threshold
    separates them; the open channels' audio is the plain run's, the closed ones' exact zeros."""
    plain = _tuner(rc, kind, floor=False)
    t = _tuner(rc, kind)
    t.set_squelch(rc.OverFloor(fm.OVER_DB))
    rise, fall = _factors(rc)
    s = np.full(fm.CELLS, np.nan, np.float32)
    for b, x in enumerate(buffers):
        plain.load(x)
        t.load(x)
        want_audio = plain.run_all()
        levels = t.levels()
        s, _ = fm.floor_run(s, t.power_spectrum(fm.CELLS), fm.HALF, fm.GUARD, 250, rise, fall, 1.0)
        thr = fm.thresholds(s, fm.channel_cells(), fm.gains(fm.OVER_DB))
        margin = float(np.min(np.abs(10.0 * np.log10(levels / thr))))
        print("%s buffer %d: nearest level %.2f dB from its threshold" % (kind, b, margin))
        assert margin >= fm.MARGIN_DB
        audio = t.run_all()
        mask = t.open_mask()
        assert np.array_equal(mask, levels >= thr) and np.array_equal(mask, STATIONS), b
        assert np.array_equal(_bits(audio[mask]), _bits(want_audio[mask])) and not _bits(audio[~mask]).any()
        if b == 0:
            assert levels[~STATIONS].max() > levels[STATIONS].min()      # a fixed threshold gets one of them wrong


def test_tuner_gate_over_floor_three_buffers(rc, buffers):
    """set_gate with OverFloor thresholds: open and close follow the floor as it drops 6 dB; the frame masks are the gate
    model's on the device's own frame levels and the model's thresholds; stations open in every frame, empty channels in none."""
    import gate_model as gm
    F = 10
    gate = rc.FrameGate(frames=F, hang=0.0, lead=0, ramp=0.0)
    t = _tuner(rc)
    t.set_gate(gate, open=rc.OverFloor(fm.OVER_DB), hysteresis_db=3.0)
    rise, fall = _factors(rc)
    s = np.full(fm.CELLS, np.nan, np.float32)
    state = np.zeros((fm.C, 2), np.int32)
    floors = []
    for b, x in enumerate(buffers):
        t.load(x)
        s, _ = fm.floor_run(s, t.power_spectrum(fm.CELLS), fm.HALF, fm.GUARD, 250, rise, fall, 1.0)
        floors.append(s)
        to = fm.thresholds(s, fm.channel_cells(), fm.gains(fm.OVER_DB))
        tc = fm.thresholds(s, fm.channel_cells(), fm.gains(fm.OVER_DB - 3.0))
        power = t.frame_levels(F)
        margin = float(np.min(np.abs(10.0 * np.log10(power / to[:, None]))))
        print("gate buffer %d: nearest frame level %.2f dB from its open threshold" % (b, margin))
        mask, any_, state = gm.gate_run(state, power, to, tc, 0, 0)
        t.run_all()
        assert np.array_equal(t.frame_mask(), mask[:, 1:].astype(bool)) and np.array_equal(t.open_mask(), any_.astype(bool)), b
        assert np.array_equal(t.frame_mask(), np.repeat(STATIONS[:, None], F, axis=1)), b
    # the state followed by `fall`: buffer 1's floor lies between the old floor and the new estimate
    assert np.all(floors[1] < floors[0]) and np.median(floors[1] / floors[0]) > DROP and np.median(floors[2] / floors[1]) < 1.0


def test_tuner_run_each_packed_drain_and_reads(rc, buffers):
    """run_each gives run_all's rows; run_all_packed through a Drain publishes the stations and nothing else."""
    t = _tuner(rc)
    t.set_squelch(rc.OverFloor(fm.OVER_DB))
    ref = _tuner(rc)
    ref.set_squelch(rc.OverFloor(fm.OVER_DB))
    pcm = rc.PCM("float32")
    drain = rc.Drain(fm.C, (fm.A, 1), pcm.dtype, depth=2)
    for b, x in enumerate(buffers[:2]):
        ref.load(x)
        want = ref.run_all()
        t.load(x)
        each = t.run_each()
        assert len(each) == fm.C and all(np.array_equal(_bits(e), _bits(w)) for e, w in zip(each, want))
        assert np.array_equal(t.open_mask(), STATIONS)
        t.run_all_packed(pcm, drain=drain)
        with drain.next() as (index, rows):
            assert index.tolist() == np.flatnonzero(STATIONS).tolist()
            assert np.array_equal(_bits(np.asarray(rows)), _bits(want[index]))
    drain.close()


def test_tuner_lanes_growing_list_and_reset(rc, buffers):
    """Lanes(depth=2) is bit-identical to the loop (the lanes share the floor's state, fenced); reset_states() unprimes the
    floor; the floor is the band's, so it carries over to a longer channel list."""
    loop = _tuner(rc)
    loop.set_squelch(rc.OverFloor(fm.OVER_DB))
    want, floors = [], []
    for x in buffers:
        loop.load(x)
        want.append(loop.run_all())
        floors.append(loop.floor())
    laned = _tuner(rc)
    laned.set_squelch(rc.OverFloor(fm.OVER_DB))
    lanes = rc.Lanes(laned, depth=2)
    tickets = [lanes.submit(x) for x in buffers]
    for b, tk in enumerate(tickets):
        audio, mask = lanes.result(tk, open_mask=True)
        assert np.array_equal(_bits(audio), _bits(want[b])) and np.array_equal(mask, STATIONS), b
    assert np.array_equal(_bits(lanes._tuners[0].floor()), _bits(floors[2])) and np.array_equal(_bits(lanes._tuners[1].floor()), _bits(floors[1]))
    # reset_states: the third buffer again, on an unprimed floor
    loop.reset_states()
    loop.load(buffers[2])
    fresh = fm.rank_filter(loop.power_spectrum(fm.CELLS), fm.HALF, fm.GUARD, 250)
    assert np.array_equal(_bits(loop.floor()), _bits(fresh)) and not np.array_equal(fresh, floors[2])
    # a growing list: the outermost channels first (the input geometry is then final), the others join with buffer 1
    order = [0, 7, 1, 2, 3, 4, 5, 6]
    grow = _tuner(rc, channels=order[:2])
    grow.set_squelch(rc.OverFloor(fm.OVER_DB))
    grow.load(buffers[0])
    grow.run_all()
    assert np.array_equal(grow.open_mask(), STATIONS[order[:2]]) and np.array_equal(_bits(grow.floor()), _bits(floors[0]))
    cs = fm.centres()
    for c in order[2:]:
        grow.add_channel(cs[c], fm.B, rc.FM(fm.B, fm.A))
        grow.request_bandwidth(float(fm.N))
    for b in (1, 2):
        grow.load(buffers[b])
        grow.run_all()
        assert np.array_equal(grow.open_mask(), STATIONS[order]), b
        assert np.array_equal(_bits(grow.floor()), _bits(floors[b])), b        # the state went on: the same floor as the loop's


class _Trace:
    """librcfm with the names of the entry points called through it."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def test_set_floor_none_restores_the_parents_path(rc, buffers):
    """With the floor off again the calls are those of a tuner that never had one, and so are the bits."""
    plain = _tuner(rc, floor=False)
    plain.set_squelch(1e-5)
    t = _tuner(rc)
    t.set_squelch(rc.OverFloor(fm.OVER_DB))
    t.load(buffers[0])
    t.run_all()
    t.set_squelch(1e-5)
    t.set_floor(None)
    plain.load(buffers[0])                                           # (both have their device handles before the trace starts)
    plain.run_all()
    plain._lib, t._lib = _Trace(plain._lib), _Trace(t._lib)
    for x in buffers[:2]:
        plain.load(x)
        t.load(x)
        assert np.array_equal(_bits(t.run_all()), _bits(plain.run_all())) and np.array_equal(t.open_mask(), plain.open_mask())
    assert t._lib.names == plain._lib.names and "rcfm_tuner_load" in t._lib.names
    assert not [n for n in t._lib.names if "floor" in n or n == "rcfm_tuner_power_spectrum"]
    with pytest.raises(RuntimeError):
        t.floor()
    # and with it on, exactly three more per load
    t.set_floor(_nf(rc))
    t._lib.names.clear()
    t.load(buffers[0])
    assert t._lib.names[-3:] == ["rcfm_tuner_power_spectrum", "rcfm_floor_run", "rcfm_floor_thresholds"]
    assert [n for n in t._lib.names if n not in plain._lib.names] == ["rcfm_tuner_power_spectrum", "rcfm_floor_run", "rcfm_floor_thresholds"]


def test_band_scan_cfar_example():
    """examples/band_scan_cfar.py at its --small geometry: the CFAR scan and the OverFloor squelch find exactly the stations in
    every second; the global median misses the weak station in the quiet part of the band at 10 dB and marks empty channels
    at the threshold that finds it."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("band_scan_cfar", os.path.join(ROOT, "examples", "band_scan_cfar.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seconds = mod.run(**mod.SMALL)
    assert len(seconds) == 3
    for r in seconds:
        air = r["on_air"]
        assert r["cfar"] == air and r["opened"] == air
        assert set(r["median"]) < set(air)                                   # stations missed, nothing else found
        assert set(air) <= set(r["median_low"]) and len(set(r["median_low"]) - set(air)) >= 5
