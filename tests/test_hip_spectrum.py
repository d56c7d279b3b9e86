"""GPU: the wideband power spectrum (rcfm_tuner_power_spectrum) against its definition in include/rcfm.h, evaluated by
tests/spectrum_model.py in float64 on the complex64 input.

Every case: max|got - exp| <= 1e-4 * max(exp) for power and for peak (the project's TOL convention, of peak), dtype and
shape, a second call bit-identical, and power with peak = NULL equal to power of the call that returns both.  Cases whose
cells all have >= 64 bins also assert the worst RELATIVE error over ALL cells, none left out, at ten times what was
measured on the MI355X against this model, rounded up to one digit.  Measured: power 5.87e-7
(N = 900 001, 1000 cells of 300 bins), so 6e-6; peak, the square of ONE bin of the float32 transform, 2.26e-6
(N = 4 000 000, span [-2 000 000, -1 929 999), 1000 cells of 70 bins), so 3e-5.
"""

import ctypes

import numpy as np
import pytest

import spectrum_model
from conftest import TOL, have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

REL_64 = {"power": 6e-6, "peak": 3e-5}      # ten times the measured worst relative error of a cell of >= 64 bins, one digit, up

# channels that give the tuner its geometry (a Tuner needs some); the spectrum call does not read them
CHANNELS = {
    90_001: [(50e6, 30000), (50.02e6, 20001)],
    900_001: [(50e6, 30000), (50.02e6, 20001)],
    4_000_000: [(100e6, 240000), (100e6 + 240000, 240000)] + [(100e6 + 366250 + 12500 * i, 12500) for i in range(8)],
    600_000: [(100e6, 240000), (100e6 + 240000, 240000)] + [(100e6 + 366250 + 12500 * i, 12500) for i in range(8)],
}


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


_loaded = {}


def _tuner(rc, N):
    """(tuner loaded with the noise-and-tones buffer of N samples, the model's shifted float64 power, mean |x|^2), one
    per N for the whole module; nothing changes them."""
    if N not in _loaded:
        t = rc.Tuner(cuda=True)
        for f, bw in CHANNELS[N]:
            t.add_channel(f, bw, None)
        t.request_bandwidth(float(N))
        x = spectrum_model.noise_and_tones(N, seed=N % 89)
        t.load(x)
        _loaded[N] = (t, spectrum_model.shifted_power(x), float(np.mean(np.abs(x.astype(np.complex128)) ** 2)))
    return _loaded[N]


def _call(handle, s0, L, M, want_power=True, want_peak=True, stream=None):
    """rcfm_tuner_power_spectrum -> (status, power, peak) as host arrays (None where not asked for)."""
    import torch
    from radiocore._internal import hip
    out = [torch.full((M,), -1.0, dtype=torch.float32, device="cuda") if w else None for w in (want_power, want_peak)]
    rc_ = hip.lib().rcfm_tuner_power_spectrum(handle, s0, L, M, hip.ptr(out[0]) if want_power else None,
                                              hip.ptr(out[1]) if want_peak else None, hip.stream() if stream is None else stream)
    torch.cuda.synchronize()
    return (rc_,) + tuple(o.cpu().numpy() if o is not None else None for o in out)


def _check(handle, P, s0, L, M, what, relative=None):
    """The assertions every case makes; returns (power, peak) of the device."""
    exp_power, exp_peak = spectrum_model.power_spectrum(P, s0, L, M)
    status, power, peak = _call(handle, s0, L, M)
    assert status == 0, (what, status)
    shortest = L // M
    relative = shortest >= 64 if relative is None else relative
    for name, got, exp in (("power", power, exp_power), ("peak", peak, exp_peak)):
        assert got.dtype == np.float32 and got.shape == (M,), (what, name, got.dtype, got.shape)
        err = float(np.max(np.abs(got - exp))) / float(np.max(exp))
        rel = float(np.max(np.abs(got - exp) / exp))
        print("%s %s: %d cells of >= %d bins, max|got - exp| / max(exp) = %.3g, worst relative error of all cells = %.3g"
              % (what, name, M, shortest, err, rel))
        assert err <= TOL, (what, name, err)
        if relative:
            assert rel <= REL_64[name], (what, name, rel)
    status, power2, peak2 = _call(handle, s0, L, M)
    assert status == 0 and np.array_equal(power, power2) and np.array_equal(peak, peak2), (what, "second call differs")
    status, alone, none = _call(handle, s0, L, M, want_peak=False)
    assert status == 0 and none is None and np.array_equal(alone, power), (what, "power with peak = NULL differs")
    status, none, alone = _call(handle, s0, L, M, want_power=False)
    assert status == 0 and none is None and np.array_equal(alone, peak), (what, "peak with power = NULL differs")
    return power, peak


# ---- the shapes: the smallest at which each hazard exists ----------------------------------------------------------

@pytest.mark.parametrize("M", [1, 7, 90_001, 1406])
def test_odd_n_full_span(rc, M):
    """N = 90 001 (odd N, 45 000 bins below zero and 45 001 from it): one cell (11 segments), seven (two segments each),
    one bin per cell (a thread per cell), and 1406 cells of 64 and 65 bins (a wave per cell)."""
    N = 90_001
    t, P, _ = _tuner(rc, N)
    _check(t._handle.value, P, -(N // 2), N, M, "N=%d M=%d" % (N, M))


@pytest.mark.parametrize("M", [3, 1000])
def test_span_across_zero_beyond_the_halo(rc, M):
    """N = 900 001, span [-150 000, +150 001): L is odd; with M = 3 the cells have 100 000 bins (13 segments) and the
    middle one straddles signed bin 0 far beyond the halo, two runs of memory in one workgroup's piece."""
    t, P, _ = _tuner(rc, 900_001)
    _check(t._handle.value, P, -150_000, 300_001, M, "N=900001 M=%d" % M)


@pytest.mark.parametrize("s0,L,M", [
    (-1_000_000, 1_000_001, 100),      # s0 even ...
    (-999_999, 1_000_001, 100),        # ... and odd with the same L: both alignments of the 16-byte body
    (2_000_000 - 70_000, 70_000, 5),   # ends exactly at N - floor(N / 2)
    (-2_000_000, 70_001, 1000),        # starts exactly at -floor(N / 2)
    (-5, 11, 11),                      # shorter than one vector per thread, across zero inside the halo
    (-5, 11, 2),
    (-3001, 6000, 2),                  # two cells of 3000 bins, a workgroup each; the second straddles zero
])
def test_spans_of_4m(rc, s0, L, M):
    t, P, _ = _tuner(rc, 4_000_000)
    _check(t._handle.value, P, s0, L, M, "N=4000000 [%d, +%d) M=%d" % (s0, L, M))


def test_one_bin_per_cell_4m(rc):
    """M = L = 4 000 000 over the full span, of-peak, and the cells' sum against mean(|x|^2) to 1e-5 relative."""
    N = 4_000_000
    t, P, mean_power = _tuner(rc, N)
    power, peak = _check(t._handle.value, P, -(N // 2), N, N, "N=4000000 M=L")
    assert np.array_equal(power, peak)
    total = float(np.sum(power.astype(np.float64)))
    assert abs(total - mean_power) <= 1e-5 * mean_power, (total, mean_power)


def test_general_form_geometry_600k(rc):
    """N = 600 000 (the tuner geometry whose levels take the general, halo-less form), full span, 1024 cells."""
    N = 600_000
    t, P, _ = _tuner(rc, N)
    _check(t._handle.value, P, -(N // 2), N, 1024, "N=600000 M=1024")


# ---- readiness -----------------------------------------------------------------------------------------------------

def _grid_tuner(rc, N, C, B):
    import workloads
    t = rc.Tuner(cuda=True)
    for f in workloads.channel_grid(C, B):
        t.add_channel(f, B, None)
    t.request_bandwidth(float(N))
    return t


def _signed(N, fb, nb):
    """The physical window [fb, fb + nb) as a signed span; the windows used here do not wrap and lie on one side of 0."""
    assert fb + nb <= N
    s0 = fb - N if fb >= N - N // 2 else fb
    assert -(N // 2) <= s0 and s0 + nb <= N - N // 2 and (s0 >= 0 or s0 + nb <= 0), (fb, nb)
    return s0


def test_readiness_shard_window_and_streams(rc):
    """RCFM_ERR_STATE before the first load; after shard + load and through window_slot / attach_window / adopt a span
    inside Tuner.window() matches the model and a span one bin beyond it on either side is refused; bad arguments are
    RCFM_ERR_ARG; a call on a second stream is bit-identical to the default stream's."""
    import torch
    from radiocore._internal import hip
    lib = hip.lib()
    N, B, C = 2_000_000, 25000, 64
    first, count = 40, 16          # clear of the band centre: their bins do not wrap around bin 0
    x = spectrum_model.noise_and_tones(N, seed=17)
    P = spectrum_model.shifted_power(x)
    whole = _grid_tuner(rc, N, C, B)
    assert _call(whole._device_tuner(N), -100, 200, 10)[0] == -5                    # before a load
    whole.load(x)
    h = whole._handle.value
    base_power, base_peak = _check(h, P, -(N // 2), N, 4000, "whole")
    for s0, L, M, pw in ((0, 0, 1, True), (0, 10, 0, True), (0, 10, 11, True), (-(N // 2) - 1, 10, 1, True),
                         (N - N // 2 - 9, 10, 1, True), (0, N + 1, 1, True), (0, 10, 1, False)):
        assert _call(h, s0, L, M, want_power=pw, want_peak=pw)[0] == -4, (s0, L, M, pw)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        status, power, peak = _call(h, -(N // 2), N, 4000, stream=hip.stream())
    assert status == 0 and np.array_equal(power, base_power) and np.array_equal(peak, base_peak)

    sharded = _grid_tuner(rc, N, C, B)
    sharded.shard(first, count)
    sharded.load(x)
    fb, nb = sharded.window(N, first, count)
    assert nb < N, "the shard's window must be a part of the spectrum"
    s0 = _signed(N, fb, nb)
    hs = sharded._handle.value
    inside, _ = _check(hs, P, s0, nb, 37, "shard")
    assert _call(hs, s0 - 1, nb + 1, 37)[0] == -5 and _call(hs, s0, nb + 1, 37)[0] == -5
    assert _call(hs, -(N // 2), N, 37)[0] == -5

    win = _grid_tuner(rc, N, C, B)
    win.shard(first, count)
    slot = win.window_slot(N, first, count)
    assert slot is not None, "these channels' window must fit a window slot"
    assert win.window(N, first, count) == (fb, nb)
    win.attach_window(slot, N)
    assert _call(win._handle.value, s0, nb, 37)[0] == -5                             # attached, not yet adopted
    X = ctypes.c_void_p()
    hip.check(lib.rcfm_tuner_spectrum(h, ctypes.byref(X)))
    hip.check(lib.rcfm_memcpy_d2d(ctypes.c_void_p(slot.data_ptr() + 8 * slot.rcfm_halo), ctypes.c_void_p(X.value + 8 * fb),
                                  ctypes.c_size_t(8 * nb), hip.stream()))
    win.adopt(N, first, count)
    hw = win._handle.value
    got, _ = _check(hw, P, s0, nb, 37, "window")
    assert np.array_equal(got, inside)                    # the same bins, the same order of the sums
    assert _call(hw, s0 - 1, nb + 1, 37)[0] == -5 and _call(hw, s0, nb + 1, 37)[0] == -5

    att = _grid_tuner(rc, N, C, B)
    att.attach(att.spectrum_slot(N), N)
    att.load(x)
    got, _ = _check(att._handle.value, P, -(N // 2), N, 4000, "attached slot")
    assert np.array_equal(got, base_power)


# ---- Python --------------------------------------------------------------------------------------------------------

def test_tuner_method(rc):
    import torch
    N = 4_000_000
    t, P, _ = _tuner(rc, N)
    f_in = t.input_frequency
    from radiocore.tools import spectrum
    s0, L = spectrum.span_bins(f_in, N, f_in - 400_000.4, f_in + 300_000.3)
    assert (s0, L) == (-400_000, 700_000)
    power, peak = t.power_spectrum(350, f_in - 400_000.4, f_in + 300_000.3, peak=True)
    exp_power, exp_peak = spectrum_model.power_spectrum(P, s0, L, 350)
    for name, got, exp in (("power", power, exp_power), ("peak", peak, exp_peak)):
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (350,)
        assert float(np.max(np.abs(got - exp))) <= TOL * float(np.max(exp))
        assert float(np.max(np.abs(got - exp) / exp)) <= REL_64[name]
    alone = t.power_spectrum(350, f_in - 400_000.4, f_in + 300_000.3)
    assert isinstance(alone, np.ndarray) and np.array_equal(alone, power)
    full = t.power_spectrum(1000)
    assert np.array_equal(full, _call(t._handle.value, -(N // 2), N, 1000)[1])
    dev = t.power_spectrum(350, f_in - 400_000.4, f_in + 300_000.3, peak=True, numpy_output=False)
    assert all(isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float32 for d in dev)
    assert np.array_equal(dev[0].cpu().numpy(), power) and np.array_equal(dev[1].cpu().numpy(), peak)
    for kw in (dict(cells=0), dict(cells=11, f_lo=f_in, f_hi=f_in + 10), dict(cells=1, f_lo=f_in + 5, f_hi=f_in + 5),
               dict(cells=1, f_lo=f_in - N, f_hi=f_in), dict(cells=1, f_lo=f_in, f_hi=f_in + N)):
        with pytest.raises(ValueError):
            t.power_spectrum(**kw)
    fresh = rc.Tuner(cuda=True)
    fresh.add_channel(100e6, 25000, None)
    with pytest.raises(RuntimeError):
        fresh.power_spectrum(10)


# ---- the example ---------------------------------------------------------------------------------------------------

def test_band_scan_example():
    """examples/band_scan.py --small finds exactly the stations it put on the air, and `occupied` at the example's own
    setting (OVER_FLOOR_DB over the median of CELL-wide cells) on the MODEL's float64 spectrum of the same buffer finds the
    same set."""
    import importlib.util
    import os
    from conftest import ROOT
    from radiocore.tools import spectrum
    spec = importlib.util.spec_from_file_location("band_scan", os.path.join(ROOT, "examples", "band_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CELL == 6250 and mod.OVER_FLOOR_DB == 10.0
    found, planted, runs, x, f_in = mod.run(**mod.SMALL)
    assert len(planted) == mod.SMALL["stations"] and found == planted
    N = x.shape[0]
    cells = N // mod.CELL
    power, _ = spectrum_model.power_spectrum(spectrum_model.shifted_power(x), -(N // 2), N, cells)
    model_runs = spectrum.occupied(power, mod.OVER_FLOOR_DB)
    assert model_runs == runs
    assert mod.channels_of(model_runs, N, cells, mod.SMALL["channels"]) == planted
