"""GPU: raw integer IQ (rcfm_iq_convert, rcfm_tuner_load_raw, Tuner.load_raw) against the complex64 path, BIT FOR BIT.

Every conversion is exact in float32 (tests/test_iq_model.py), and behind the conversion both paths run the same template
code on the same values, so nothing here has a tolerance: torch.equal on the bit patterns, and no NaN left of the NaN the
storage is refilled with before each load (a load that stores nothing must fail, not repeat the other's result).

Sizes of the load comparison, by what rcfm_fft_describe reports (each test asserts it and prints the route):
  N = 240         outside the engine (below 256): rocFFT, route 0.  The issue's "N = 480, one pass" does not exist: the engine
                  plans two passes or more for every length it takes (480 = 16 x 30), so the nearest length that has no
                  first pass to ride on is the largest smooth one below 256;
  N = 480         two passes of lengths without a compile-time tile (16 x 30): the runtime-radix kernel, route 1;
  N = 240 000     two passes (480 x 500, padded scratch rows), route 1;
  N = 2 400 000   three passes (120 x 125 x 160), cache-resident, plain hand-over, in-place middle pass, route 1;
  N = 90 001      rocFFT, route 0;
  N = 2.4e8       three big tiles, beyond the Infinity Cache: default plan (600 x 625 x 640: tile-blocked hand-over, ping-pong)
                  and aligned plan (640 x 625 x 600: flat XCD-aware first pass, two scratch arrays), route 1.
"""

import ctypes
import importlib.util
import os

import numpy as np
import pytest

import iq_model
from conftest import ROOT, have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

FORMATS = [iq_model.RCFM_IQ_CS16, iq_model.RCFM_IQ_CS8, iq_model.RCFM_IQ_CU8]
ERR_ARG, ERR_STATE = -4, -5


def _env():
    import torch
    from radiocore._internal import hip
    return torch, hip, hip.lib()


def _torch_dtype(fmt):
    import torch
    return {iq_model.RCFM_IQ_CS16: torch.int16, iq_model.RCFM_IQ_CS8: torch.int8, iq_model.RCFM_IQ_CU8: torch.uint8}[fmt]


def _bits(t):
    import torch
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _assert_same_bits(got, want, what):
    import torch
    assert not bool(torch.isnan(torch.view_as_real(got)).any()), "%s: the raw load left part of the storage unwritten" % what
    assert torch.equal(_bits(got), _bits(want)), "%s: differs from the complex64 path" % what


def _nan_fill(t):
    import torch
    torch.view_as_real(t).fill_(float("nan"))


def _plan(n):
    """rcfm_fft_describe's plan of length n, or None when the length runs on rocFFT."""
    _, hip, lib = _env()
    plan = hip.FftPlan()
    return plan if lib.rcfm_fft_describe(n, 0, ctypes.byref(plan)) == 0 else None


def _handle(n, rolls, bws):
    _, hip, lib = _env()
    t = ctypes.c_void_p()
    hip.check(lib.rcfm_tuner_create(n, len(rolls), (ctypes.c_int64 * len(rolls))(*rolls), (ctypes.c_int32 * len(bws))(*bws),
                                    ctypes.byref(t)))
    return hip.Handle(t, lib.rcfm_tuner_destroy)


def _layout(t):
    _, hip, lib = _env()
    halo, nn = ctypes.c_int64(), ctypes.c_int64()
    hip.check(lib.rcfm_tuner_spectrum_layout(t.value, ctypes.byref(halo), ctypes.byref(nn)))
    return int(halo.value), int(nn.value)


def _route(t, fmt):
    _, hip, lib = _env()
    r = ctypes.c_int(-1)
    hip.check(lib.rcfm_tuner_load_route(t.value, fmt, ctypes.byref(r)))
    return int(r.value)


def _attached_slot(t):
    torch, hip, lib = _env()
    halo, n = _layout(t)
    slot = hip.empty((n + 2 * halo,), torch.complex64)
    hip.check(lib.rcfm_tuner_attach_spectrum(t.value, hip.ptr(slot), 0, 0))
    return slot, halo


def _load(t, fmt, buf):
    """rcfm_tuner_load (fmt 0) or rcfm_tuner_load_raw of a device tensor; returns the status."""
    _, hip, lib = _env()
    if fmt == 0:
        return lib.rcfm_tuner_load(t.value, hip.ptr(buf), hip.stream())
    return lib.rcfm_tuner_load_raw(t.value, fmt, hip.ptr(buf), hip.stream())


def _host_case(fmt, n, seed):
    """(raw int device tensor [n, 2], converted complex64 device tensor [n]) with the extremes planted (iq_model)."""
    torch, _, _ = _env()
    plan = _plan(n)
    line = n // plan.passes[0].L if plan is not None else 16      # point 1 of the first pass's first tile: its second line
    raw = iq_model.random_pairs(fmt, n, seed, line=line)
    return torch.from_numpy(raw).cuda(), torch.from_numpy(iq_model.to_complex64(raw)).cuda()


# ---- 1. the conversion alone ------------------------------------------------------------------------------------------

def _every_value(fmt):
    dt = iq_model.DTYPES[fmt]
    v = iq_model.all_values(dt)
    if fmt == iq_model.RCFM_IQ_CS16:            # all 65 536 values as I against a shuffled copy as Q
        return np.stack([v, np.random.default_rng(16).permutation(v)], axis=1)
    i, q = np.meshgrid(v, v, indexing="ij")     # all 256 x 256 pairs
    return np.stack([i.reshape(-1), q.reshape(-1)], axis=1)


def _convert(fmt, raw, in_offset, out_offset):
    """rcfm_iq_convert of raw [n, 2] placed `in_offset` integers behind a 16-byte boundary, into an output `out_offset`
    complex64 elements behind one; the elements around the output must stay untouched."""
    torch, hip, lib = _env()
    n = raw.shape[0]
    src = torch.zeros(2 * n + in_offset + 8, dtype=_torch_dtype(fmt), device="cuda")
    dst = hip.empty((n + out_offset + 2,), torch.complex64)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    src[in_offset:in_offset + 2 * n] = torch.from_numpy(raw.reshape(-1)).cuda()
    _nan_fill(dst)
    hip.check(lib.rcfm_iq_convert(fmt, ctypes.c_size_t(n), ctypes.c_void_p(src.data_ptr() + in_offset * raw.itemsize),
                                  ctypes.c_void_p(dst.data_ptr() + 8 * out_offset), hip.stream()))
    torch.cuda.synchronize()
    guard = torch.cat([dst[:out_offset], dst[out_offset + n:]])
    assert bool(torch.isnan(torch.view_as_real(guard)).all()), "rcfm_iq_convert wrote outside [0, n)"
    return dst[out_offset:out_offset + n]


@pytest.mark.parametrize("fmt", FORMATS)
def test_convert_every_value_against_the_model(fmt):
    torch, _, _ = _env()
    raw = _every_value(fmt)
    assert raw.shape == (65536, 2)
    want = torch.from_numpy(iq_model.to_complex64(raw)).cuda()
    assert torch.equal(_bits(_convert(fmt, raw, 0, 0)), _bits(want))


@pytest.mark.parametrize("n", [1, 3, 65537])
@pytest.mark.parametrize("fmt", FORMATS)
def test_convert_odd_counts_and_offsets(fmt, n):
    """n = 1, 3, 65 537; the input one I, Q pair behind a 16-byte boundary and, once more, one INTEGER behind it (the
    header asks for the integer's natural alignment only); the output 8 bytes behind a 16-byte boundary, and aligned."""
    torch, _, _ = _env()
    raw = np.concatenate([_every_value(fmt), _every_value(fmt)[:1]])[:n] if n > 3 else iq_model.random_pairs(fmt, n, n)
    want = torch.from_numpy(iq_model.to_complex64(raw)).cuda()
    for in_offset, out_offset in ((2, 1), (1, 1), (1, 0)):
        got = _convert(fmt, raw, in_offset, out_offset)
        assert torch.equal(_bits(got), _bits(want)), (in_offset, out_offset)


def test_convert_through_python():
    torch, _, _ = _env()
    from radiocore.tools import iq
    raw = iq_model.random_pairs(iq_model.RCFM_IQ_CS16, 1001, 5)
    want = torch.from_numpy(iq_model.to_complex64(raw)).cuda()
    for arg in (raw, raw.reshape(-1), torch.from_numpy(raw).cuda()):
        got = iq.to_complex64(arg)
        assert got.dtype == torch.complex64 and got.is_cuda and torch.equal(_bits(got), _bits(want))


# ---- 2. rcfm_tuner_load_raw against rcfm_tuner_load of the converted buffer ---------------------------------------------

# n: (passes rcfm_fft_describe reports or None for rocFFT, route, channel bandwidth)
LOAD_SIZES = {240: (None, 0, 32), 480: (2, 1, 32), 240_000: (2, 1, 12_000), 2_400_000: (3, 1, 60_000), 90_001: (None, 0, 5_000)}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", sorted(LOAD_SIZES))
def test_load_raw_equals_load_of_the_converted_buffer(n, fmt):
    torch, hip, lib = _env()
    passes, route, bw = LOAD_SIZES[n]
    plan = _plan(n)
    assert (plan.npass if plan is not None else None) == passes
    if n == 2_400_000:      # cache-resident, plain hand-over
        assert n * 8 <= (256 << 20) and plan.passes[0].out_t == 0
    t = _handle(n, [0, n // 3, -(n // 4)], [bw] * 3)
    assert _route(t, fmt) == route
    slot, halo = _attached_slot(t)
    assert halo > 0
    raw, wide = _host_case(fmt, n, n + fmt)
    print("N = %d %s: %s, route %d, halo %d" % (n, iq_model.NAMES[fmt],
                                                "rocFFT" if plan is None else " x ".join(str(plan.passes[i].L) for i in range(plan.npass)),
                                                route, halo))
    _nan_fill(slot)
    hip.check(_load(t, fmt, raw))
    got = slot.clone()
    _nan_fill(slot)
    hip.check(_load(t, 0, wide))
    torch.cuda.synchronize()
    _assert_same_bits(got, slot, "N = %d %s" % (n, iq_model.NAMES[fmt]))


@pytest.mark.parametrize("aligned", [1, 0])
@pytest.mark.parametrize("fmt", [iq_model.RCFM_IQ_CS16, iq_model.RCFM_IQ_CS8])
def test_load_raw_at_the_wideband_size(fmt, aligned):
    """N = 2.4e8 with cfg4's channel list (1024 channels of 240 kHz on a 200 kHz raster) on the handle's own storage, which the
    aligned plan needs: the big tiles, the flat first pass (aligned), ping-pong and the tile-blocked hand-over (default)."""
    torch, hip, lib = _env()
    n, C, B, raster = 240_000_000, 1024, 240_000, 200_000
    plan = _plan(n)
    assert plan.npass == 3 and [plan.passes[i].L for i in range(3)] == [600, 625, 640] and plan.passes[0].out_t != 0
    t = _handle(n, [-int((i - (C - 1) / 2.0) * raster) for i in range(C)], [B] * C)
    hip.check(lib.rcfm_tuner_set_option(t.value, hip.RCFM_TUNER_OPT_ALIGNED_PLAN, aligned))
    assert _route(t, fmt) == 1
    halo, _ = _layout(t)
    info = np.iinfo(iq_model.DTYPES[fmt])
    g = torch.Generator(device="cuda").manual_seed(240 + fmt)
    raw = torch.randint(info.min, info.max + 1, (n, 2), generator=g, device="cuda", dtype=torch.int32).to(
        _torch_dtype(fmt))
    first_len = 640 if aligned else 600
    for k, s in enumerate((0, 1, n - 1, n // first_len)):
        raw[s, 0], raw[s, 1] = (info.min, info.max) if k % 2 == 0 else (info.max, info.min)
    wide = hip.empty((n,), torch.complex64)
    hip.check(lib.rcfm_iq_convert(fmt, ctypes.c_size_t(n), hip.ptr(raw), hip.ptr(wide), hip.stream()))
    X = ctypes.c_void_p()
    hip.check(lib.rcfm_tuner_spectrum(t.value, ctypes.byref(X)))
    storage = ctypes.c_void_p(X.value - 8 * halo)                   # [halo | n | halo]
    nbytes = ctypes.c_size_t(8 * (n + 2 * halo))
    nans = hip.empty((n + 2 * halo,), torch.complex64)
    _nan_fill(nans)
    copies = []
    for f, buf in ((fmt, raw), (0, wide)):
        hip.check(lib.rcfm_memcpy_d2d(storage, hip.ptr(nans), nbytes, hip.stream()))
        hip.check(_load(t, f, buf))
        c = hip.empty((n + 2 * halo,), torch.complex64)
        hip.check(lib.rcfm_memcpy_d2d(hip.ptr(c), storage, nbytes, hip.stream()))
        copies.append(c)
    torch.cuda.synchronize()
    print("N = 2.4e8 %s, aligned plan %d: route 1, halo %d" % (iq_model.NAMES[fmt], aligned, halo))
    _assert_same_bits(copies[0], copies[1], "N = 2.4e8 %s aligned %d" % (iq_model.NAMES[fmt], aligned))


# ---- 3. sharded load ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_sharded_load_raw(fmt):
    torch, hip, lib = _env()
    n, B, C = 2_400_000, 60_000, 14
    t = _handle(n, [-(300_000 + 140_000 * c) for c in range(C)], [B] * C)       # channel c sits at bin 300 000 + 140 000 c
    first, count = 4, 3
    hip.check(lib.rcfm_tuner_shard(t.value, first, count))
    fb, nb = ctypes.c_int64(), ctypes.c_int64()
    hip.check(lib.rcfm_tuner_window(t.value, first, count, ctypes.byref(fb), ctypes.byref(nb)))
    fb, nb = int(fb.value), int(nb.value)
    assert 0 < nb < n, "the shard keeps the whole spectrum: nothing is tested"
    slot, halo = _attached_slot(t)
    raw, wide = _host_case(fmt, n, 33 + fmt)
    held = (fb + torch.arange(nb, device="cuda")) % n + halo
    results = []
    for f, buf in ((fmt, raw), (0, wide)):
        _nan_fill(slot)
        hip.check(_load(t, f, buf))
        out = hip.empty((count, B), torch.complex64)
        hip.check(lib.rcfm_tuner_run(t.value, first, count, hip.ptr(out), hip.stream()))
        assert lib.rcfm_tuner_run(t.value, first + count, 1, hip.ptr(out[:1].clone()), hip.stream()) == ERR_STATE
        assert lib.rcfm_tuner_run(t.value, 0, 1, hip.ptr(out[:1].clone()), hip.stream()) == ERR_STATE
        torch.cuda.synchronize()
        results.append((slot[held].clone(), out))
    print("N = %d %s sharded to channels [%d, %d): route %d, %d of %d bins held" % (n, iq_model.NAMES[fmt], first, first + count,
                                                                                 _route(t, fmt), nb, n))
    _assert_same_bits(results[0][0], results[1][0], "held bins")
    _assert_same_bits(results[0][1], results[1][1], "rcfm_tuner_run of the shard")


# ---- 4. through Python -------------------------------------------------------------------------------------------------

PY_N, PY_C, PY_B, PY_A, PY_BUFFERS = 2_000_000, 24, 25_000, 8_000, 3


def _py_tuner(kind):
    import radiocore as rc
    import workloads
    t = rc.Tuner()
    for f in workloads.channel_grid(PY_C, 75_000):
        t.add_channel(f, PY_B, getattr(rc, kind)(PY_B, PY_A))
    t.request_bandwidth(float(PY_N))
    return t


@pytest.fixture(scope="module")
def py_buffers():
    """Three int16 buffers [N, 2] (a station per channel, quantised at 90 % of full scale) and their complex64 conversions."""
    import workloads
    centres = workloads.channel_grid(PY_C, 75_000)
    x = workloads.wideband(PY_N, (min(centres) + max(centres)) / 2, centres, PY_B, gain=0.1, stereo=False)
    iq = x.view(np.float32).reshape(-1, 2)
    base = np.rint(iq * (0.9 * 32767.0 / float(np.max(np.abs(iq))))).astype(np.int16)
    raw = [np.ascontiguousarray(np.roll(base, 3111 * b, axis=0)) for b in range(PY_BUFFERS)]
    return raw, [iq_model.to_complex64(r) for r in raw]


@pytest.fixture(scope="module")
def py_reference(py_buffers):
    """{kind: ([audio per buffer], [levels per buffer])} of Tuner.load of the converted arrays, one buffer at a time."""
    ref = {}
    for kind in ("AM", "FM"):
        t = _py_tuner(kind)
        audio, levels = [], []
        for w in py_buffers[1]:
            t.load(w)
            audio.append(t.run_all())
            levels.append(t.levels())
        ref[kind] = (audio, levels)
    return ref


@pytest.mark.parametrize("kind", ["AM", "FM"])
def test_python_load_raw_run_all_and_levels(kind, py_buffers, py_reference):
    _, hip, lib = _env()
    t = _py_tuner(kind)
    for b, raw in enumerate(py_buffers[0]):
        t.load_raw(raw if b != 1 else raw.reshape(-1))             # [N, 2] and [2 N]
        assert np.array_equal(t.run_all(), py_reference[kind][0][b]), b
        assert np.array_equal(t.levels(), py_reference[kind][1][b]), b
    r = ctypes.c_int(-1)
    hip.check(lib.rcfm_tuner_load_route(t._handle.value, hip.RCFM_IQ_CS16, ctypes.byref(r)))
    print("Tuner.load_raw(int16), N = %d, %s: route %d" % (PY_N, kind, r.value))
    assert r.value == 1
    assert float(np.max(np.abs(py_reference[kind][0][0]))) > 0


@pytest.mark.parametrize("kind", ["AM", "FM"])
def test_python_lanes_submit_raw(kind, py_buffers, py_reference):
    from radiocore.tools import Lanes
    lanes = Lanes(_py_tuner(kind), depth=2)
    tickets = [lanes.submit(raw, raw=True) for raw in py_buffers[0]]
    for b, tk in enumerate(tickets):
        assert np.array_equal(lanes.result(tk), py_reference[kind][0][b]), b


def test_python_feeder_int16_into_load_raw(py_buffers, py_reference):
    from radiocore.tools import Buffer, Feeder
    t = _py_tuner("AM")
    host = []
    for raw in py_buffers[0]:
        b = Buffer(2 * PY_N, "int16", cuda=True)                  # page-locked
        b.data[:] = raw.reshape(-1)
        host.append(b)
    feeder = Feeder(2 * PY_N, "int16")
    feeder.submit(host[0].data)
    for i in range(PY_BUFFERS):
        if i + 1 < PY_BUFFERS:
            feeder.submit(host[i + 1].data)
        with feeder.next() as x:
            t.load_raw(x)
            audio = t.run_all()
        assert np.array_equal(audio, py_reference["AM"][0][i]), i
    feeder.close()
    with pytest.raises(ValueError):
        Feeder(2 * PY_N, "int16").submit(host[0].data.view(np.uint16))


def test_airband_cs16_example():
    """examples/airband_cs16.py at a reduced size: the audio of the int16 loop is that of the complex64 loop."""
    spec = importlib.util.spec_from_file_location("airband_cs16", os.path.join(ROOT, "examples", "airband_cs16.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    identical, audio, host_ms = mod.run(channels=120, rate=4_000_000, seconds=2)
    assert identical is True
    assert len(audio) == 2 and audio[0].shape == (120, mod.AUDIO, 1) and float(np.max(np.abs(audio[0]))) > 0.1
    assert not np.array_equal(audio[0], audio[1])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------

def test_python_refusals(py_buffers):
    t = _py_tuner("AM")
    raw = py_buffers[0][0]
    for bad in (raw.astype(np.float16), raw.astype(np.int32), raw.reshape(-1)[:-1], raw[:-2], raw.reshape(-1, 4)):
        with pytest.raises(ValueError):
            t.load_raw(bad)
    with pytest.raises(ValueError, match="input_sig size and input_size mismatch"):
        t.load_raw(raw[:PY_N // 2])
    with pytest.raises(RuntimeError, match="before Tuner.load"):
        t.run(0)                                                  # nothing above was loaded
    t.load_raw(raw)
    assert t.run(0).shape == (PY_B,)


def test_load_raw_is_refused_while_a_window_is_attached():
    torch, hip, lib = _env()
    n, B, C = 2_400_000, 60_000, 14
    t = _handle(n, [-(300_000 + 140_000 * c) for c in range(C)], [B] * C)
    halo, nb = ctypes.c_int64(), ctypes.c_int64()
    hip.check(lib.rcfm_tuner_window_layout(t.value, 4, 3, ctypes.byref(halo), ctypes.byref(nb)))
    window = hip.empty((int(nb.value) + 2 * int(halo.value),), torch.complex64)
    hip.check(lib.rcfm_tuner_attach_window(t.value, hip.ptr(window), 4, 3))
    raw, wide = _host_case(iq_model.RCFM_IQ_CS16, n, 9)
    assert _load(t, 0, wide) == ERR_STATE
    for fmt in FORMATS:
        assert _load(t, fmt, raw) == ERR_STATE
    for fmt in (0, 4):
        assert lib.rcfm_tuner_load_raw(t.value, fmt, hip.ptr(raw), hip.stream()) == ERR_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [90_001, 240_000])
def test_load_and_load_raw_alternate_on_one_handle(n):
    """load after load_raw and the reverse, on both routes: every spectrum is the right one -- at N = 90 001 the scratch the
    conversion fills (route 0) aliases nothing the complex64 load uses."""
    torch, hip, lib = _env()
    fmt = iq_model.RCFM_IQ_CS16
    t = _handle(n, [0, n // 3, -(n // 4)], [LOAD_SIZES[n][2]] * 3)
    slot, _ = _attached_slot(t)
    cases = [_host_case(fmt, n, seed) for seed in (1, 2)]
    want = []
    for raw, wide in cases:                           # the complex64 load of each buffer, before any raw load on this handle
        _nan_fill(slot)
        hip.check(_load(t, 0, wide))
        want.append(slot.clone())
    assert not torch.equal(_bits(want[0]), _bits(want[1]))
    print("N = %d: route %d" % (n, _route(t, fmt)))
    assert _route(t, fmt) == LOAD_SIZES[n][1]
    for k, f in ((0, fmt), (1, 0), (0, fmt), (0, 0), (1, fmt), (0, 0)):
        _nan_fill(slot)
        hip.check(_load(t, f, cases[k][0] if f else cases[k][1]))
        torch.cuda.synchronize()
        _assert_same_bits(slot, want[k], "buffer %d, format %d" % (k, f))
