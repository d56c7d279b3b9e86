"""GPU: the batched single-stage entry points of include/rcfm.h (rcfm_resampler_*, rcfm_filtfilt, rcfm_lfilter_fir,
rcfm_hilbert, rcfm_pll_phase, rcfm_discriminator) through hip.lib() directly, at C > 1 and at the sizes, parities and
tap counts where their kernels branch, against the float64 references of tests/primitives_model.py.

Every comparison is per row (max|delta_c| / max|ref_c|, worst row) and is held to primitives_model.gpu_bound(): four
times the error of the same mathematics in float32 on the CPU (tests/test_primitives_model.py pins that), never more
than conftest.TOL.  Routes are read from rcfm_fft_describe, never assumed.

What the library does at the edges (recorded, and asserted below):
    rcfm_lfilter_fir with y == x is refused (RCFM_ERR_ARG): the final state is built from x after y is written.
    rcfm_pll_phase far outside primitives_model.pll_magnitude_range: the multiply-out branch overflows / underflows
    like numpy's complex64 power -- NaN everywhere; the principal branch uses arg z alone and stays finite where
    numpy's power is NaN.  z = 0 is NaN on both branches, except mult = 0 where, like numpy's, the power is 1.
    C > 65535, more taps than the kernels' LDS holds (filtfilt 2867, lfilter 5461): RCFM_ERR_ARG, nothing launched.

Worst measured error / bound on an MI355X (worst row of every case of the entry point):
    rcfm_resampler_*, complex   1.05e-6 / 2.4e-6   (the prime length 10007 through rocFFT; engine routes <= 5.8e-7)
    rcfm_resampler_*, real      3.9e-7  / 1.8e-6
    rcfm_filtfilt               7.8e-7  / 1.24e-6  (head 7.8e-7, interior 7.5e-7, tail 7.2e-7; the ramp: 9.9e-7)
    rcfm_lfilter_fir, outputs   2.1e-7  / 9.2e-7
    rcfm_lfilter_fir, state     7.0e-7  / 1.24e-6
    rcfm_hilbert                9.6e-7  / 2.4e-6   (Re z against x: 9.6e-7)
    rcfm_discriminator          1.8e-7  / 6.8e-7
    rcfm_pll_phase (absolute)   mult 1, 2, 3: 1.6e-7 / 8.2e-7 .. 8.6e-7; 7: 2.0e-7 / 1.5e-6; 64: 6.5e-7 / 1.7e-5;
                                principal branch (0.5, 2.5, 65, -1): 3.0e-8 / 8.2e-7 .. 1.8e-5; mult 0: 0 / 4.8e-7
    at the tap limits           rcfm_filtfilt, 2867 taps: 2.8e-6; rcfm_lfilter_fir, 5461 taps: 8.0e-8 (both / 1e-4)
"""
import ctypes
import os

import numpy as np
import pytest

import primitives_model as pm
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ERR_ARG = -4


@pytest.fixture(scope="module")
def rt():
    import torch
    from radiocore._internal import hip

    class RT:
        pass
    r = RT()
    r.torch, r.hip, r.lib = torch, hip, hip.lib()
    return r


def dev(rt, a):
    return rt.torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(rt, t):
    rt.torch.cuda.synchronize()
    return t.cpu().numpy()


def report(what, err, bound):
    print("%-60s %.3g (bound %.3g)" % (what, err, bound))
    return err


def engine_row_length(rt, n):
    """Row length n_1 of the engine's plan for n, or None where rcfm_fft_describe refuses the length (rocFFT then)."""
    plan = rt.hip.FftPlan()
    if rt.lib.rcfm_fft_describe(n, 0, ctypes.byref(plan)) != 0:
        return None
    assert plan.n == n
    return int(plan.passes[0].L)


def resampler_route(rt, C, n, m, cplx):
    """What rcfm_resampler_create decides, from the plan: "rocfft", "engine" or "engine-windowed" (the long
    transform stores only the rows of the spectrum the m bins lie in: one signal, rows lo .. and .. hi)."""
    assert os.environ.get("RCFM_FFT") != "rocfft", "RCFM_FFT=rocfft takes every transform off the engine"
    L = engine_row_length(rt, n)
    if not cplx or m > n or L is None or engine_row_length(rt, m) is None:
        return "rocfft", None
    nyq = m // 2 + 1
    nneg = m - nyq if m > 2 else 0
    hi, lo, rows = (nyq + 1) // L, (n - nneg - 2) // L, n // L
    return ("engine-windowed" if C == 1 and lo > hi + 1 and lo < rows else "engine"), (lo, hi, rows)


def resample(rt, x, m, handle=None):
    C, n = x.shape
    cplx = np.iscomplexobj(x)
    h = handle or ctypes.c_void_p()
    if handle is None:
        rt.hip.check(rt.lib.rcfm_resampler_create(C, n, m, int(cplx), ctypes.byref(h)))
    xd = dev(rt, x)
    yd = rt.torch.empty((C, m), dtype=xd.dtype, device="cuda")
    rt.hip.check(rt.lib.rcfm_resampler_run(h, rt.hip.ptr(xd), rt.hip.ptr(yd), rt.hip.stream()))
    y = host(rt, yd)
    if handle is None:
        rt.hip.check(rt.lib.rcfm_resampler_destroy(h))
    return y


# ---- rcfm_resampler_* ------------------------------------------------------------------------------------------------------

def nyquist_branch(n, m, cplx):
    even = min(n, m) % 2 == 0
    if cplx:
        return "NYQ_DOWN" if even and m < n and min(n, m) > 2 else "NYQ_UP" if even and n < m else "none"
    return "factor 2" if even and m < n else "factor 1/2" if even and n < m else "factor 1"


def test_the_resampler_cases_reach_every_route_and_nyquist_branch(rt):
    routes = {(resampler_route(rt, 1, n, m, True)[0], nyquist_branch(n, m, True)) for n, m in pm.RESAMPLE_COMPLEX}
    for want in [("engine-windowed", "NYQ_DOWN"), ("engine", "none"), ("rocfft", "NYQ_DOWN"), ("rocfft", "NYQ_UP"),
                 ("rocfft", "none")]:
        assert want in routes, (want, routes)
    assert resampler_route(rt, 3, 100000, 2500, True)[0] == "engine"          # the same geometry, batched: unwindowed
    ups = [(n, m) for n, m in pm.RESAMPLE_COMPLEX if m > n]
    assert {(n % 2, m % 2) for n, m in ups} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    downs = [(n, m) for n, m in pm.RESAMPLE_COMPLEX if m < n and resampler_route(rt, 1, n, m, True)[0] == "rocfft"]
    assert {(n % 2, m % 2) for n, m in downs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(engine_row_length(rt, n) is None and n % 2 == 1 for n, _ in pm.RESAMPLE_COMPLEX)
    assert {nyquist_branch(n, m, False) for n, m in pm.RESAMPLE_REAL} == {"factor 2", "factor 1/2", "factor 1"}
    for sel in (lambda n, m: m < n, lambda n, m: m > n):
        assert {(n % 2, m % 2) for n, m in pm.RESAMPLE_REAL if sel(n, m)} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("n,m", pm.RESAMPLE_COMPLEX)
def test_resampler_complex_batches(rt, n, m):
    bound = pm.gpu_bound(pm.YARDSTICK["resample_complex"])
    worst = 0.0
    for C in pm.BATCHES:
        x = pm.spectral_input(C, n, m, True, 1)
        got = resample(rt, x, m)
        worst = max(worst, report("resampler complex %d -> %d C=%d %s" % (n, m, C, resampler_route(rt, C, n, m, True)[0]),
                                  pm.worst_row(got, pm.ref_resample(x, m)), bound))
    assert worst <= bound


@pytest.mark.parametrize("n,m", pm.RESAMPLE_REAL)
def test_resampler_real_batches(rt, n, m):
    bound = pm.gpu_bound(pm.YARDSTICK["resample_real"])
    worst = 0.0
    for C in pm.BATCHES:
        x = pm.spectral_input(C, n, m, False, 1)
        got = resample(rt, x, m)
        worst = max(worst, report("resampler real %d -> %d C=%d %s" % (n, m, C, nyquist_branch(n, m, False)),
                                  pm.worst_row(got, pm.ref_resample(x, m)), bound))
    assert worst <= bound


def test_resampler_windowed_single_signal_equals_row_0_of_the_unwindowed_batch(rt):
    n, m = 100000, 2500
    assert resampler_route(rt, 1, n, m, True)[0] == "engine-windowed"
    assert resampler_route(rt, 3, n, m, True)[0] == "engine"
    bound = pm.gpu_bound(pm.YARDSTICK["resample_complex"])
    x = pm.spectral_input(3, n, m, True, 1)
    ref = pm.ref_resample(x, m)
    one, three = resample(rt, x[:1], m), resample(rt, x, m)
    assert report("windowed C=1 vs reference", pm.worst_row(one, ref[:1]), bound) <= bound
    assert report("unwindowed C=3 vs reference", pm.worst_row(three, ref), bound) <= bound
    assert report("windowed C=1 vs row 0 of C=3", pm.worst_row(one, three[:1].astype(np.complex128)), bound) <= bound


@pytest.mark.parametrize("n,m,want", [(6000, 5880, "engine-windowed"), (12000, 11907, "engine")])
def test_resampler_at_the_edge_of_the_row_window(rt, n, m, want):
    """lo == hi + 2: one row of the long spectrum is left out; lo == hi + 1: none could be, no window."""
    route, (lo, hi, rows) = resampler_route(rt, 1, n, m, True)
    assert route == want and (lo == hi + 2 if want == "engine-windowed" else lo == hi + 1) and lo < rows, (route, lo, hi, rows)
    bound = pm.gpu_bound(pm.YARDSTICK["resample_complex"])
    for C in (1, 3):
        x = pm.spectral_input(C, n, m, True, 2)
        assert report("row window edge %d -> %d C=%d" % (n, m, C), pm.worst_row(resample(rt, x, m), pm.ref_resample(x, m)),
                      bound) <= bound


@pytest.mark.parametrize("cplx,C,n,m", [(True, 1, 100000, 2500), (True, 3, 6000, 1200), (True, 2, 1001, 200),
                                        (False, 3, 1000, 200), (False, 2, 200, 1001)])
def test_resampler_handle_keeps_nothing_between_runs(rt, cplx, C, n, m):
    bound = pm.gpu_bound(pm.YARDSTICK["resample_complex" if cplx else "resample_real"])
    h = ctypes.c_void_p()
    rt.hip.check(rt.lib.rcfm_resampler_create(C, n, m, int(cplx), ctypes.byref(h)))
    for seed in (11, 12):
        x = pm.spectral_input(C, n, m, cplx, seed)
        assert report("second run" if seed == 12 else "first run", pm.worst_row(resample(rt, x, m, h), pm.ref_resample(x, m)),
                      bound) <= bound
    rt.hip.check(rt.lib.rcfm_resampler_destroy(h))


# ---- rcfm_filtfilt ---------------------------------------------------------------------------------------------------------

def filtfilt(rt, b, x):
    C, n = x.shape
    xd = dev(rt, x)
    yd = rt.torch.empty_like(xd)
    taps, taps_p = rt.hip.float_array(b)
    rt.hip.check(rt.lib.rcfm_filtfilt(C, n, taps_p, len(taps), rt.hip.ptr(xd), rt.hip.ptr(yd), rt.hip.stream()))
    return host(rt, yd)


@pytest.mark.parametrize("kind", ["firwin", "random"])
@pytest.mark.parametrize("ntaps", pm.FILTFILT_TAPS)
def test_filtfilt_batches_sizes_and_ends(rt, kind, ntaps):
    bound = pm.gpu_bound(pm.YARDSTICK["filtfilt"])
    b = pm.filter_taps(kind, ntaps)
    worst = 0.0
    for n in pm.filtfilt_sizes(ntaps):
        for C in pm.FILTFILT_BATCHES:
            x = pm.filtfilt_input(C, n, 2)
            got, ref = filtfilt(rt, b, x), pm.ref_filtfilt(b, x)
            head, inner, tail = pm.segment_errors(got, ref, 3 * ntaps)
            print("filtfilt %s %d taps n=%d C=%d: head %.3g interior %.3g tail %.3g (bound %.3g)"
                  % (kind, ntaps, n, C, head, inner, tail, bound))
            worst = max(worst, head, inner, tail, pm.worst_row(got, ref))
            # unit DC gain and a symmetric g: the reference returns a ramp as it went in (test_primitives_model.py:
            # to 2e-7), ends included, where a wrong odd extension shows
            r = pm.ramp_rows(C, n)
            back = filtfilt(rt, b, r)
            rh, ri, rtl = pm.segment_errors(back, pm.ref_filtfilt(b, r), 3 * ntaps)
            print("          ramp: head %.3g interior %.3g tail %.3g" % (rh, ri, rtl))
            worst = max(worst, rh, ri, rtl)
            assert max(pm.segment_errors(back, r.astype(np.float64), 3 * ntaps)) <= bound + 2e-7
    assert worst <= bound, worst


def test_filtfilt_refuses_the_length_scipy_refuses(rt):
    for ntaps in pm.FILTFILT_TAPS:
        n = 3 * ntaps
        b = pm.filter_taps("firwin", ntaps)
        xd = dev(rt, pm.noise_rows(1, n, 1))
        taps, taps_p = rt.hip.float_array(b)
        st = rt.lib.rcfm_filtfilt(1, n, taps_p, ntaps, rt.hip.ptr(xd), rt.hip.ptr(rt.torch.empty_like(xd)), rt.hip.stream())
        assert st == ERR_ARG
        want = "The length of the input vector x must be greater than padlen, which is %d." % n
        assert rt.lib.rcfm_last_error().decode() == want
        with pytest.raises(ValueError) as e:
            pm.ref_filtfilt(b, np.ones((1, n)))
        assert str(e.value) == want


# ---- rcfm_lfilter_fir ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ntaps", pm.LFILTER_TAPS)
@pytest.mark.parametrize("C", pm.LFILTER_BATCHES)
def test_lfilter_three_consecutive_buffers_and_the_final_state(rt, C, ntaps):
    b = pm.filter_taps("random", ntaps, seed=3)
    taps, taps_p = rt.hip.float_array(b)
    by, bz = pm.gpu_bound(pm.YARDSTICK["lfilter"]), pm.gpu_bound(pm.YARDSTICK["lfilter_state"])
    worst_y = worst_z = 0.0
    for n in pm.lfilter_sizes(ntaps):
        x, zi = pm.lfilter_input(C, n, ntaps, pm.LFILTER_BUFFERS, 4)
        state = dev(rt, zi) if ntaps > 1 else None
        got = []
        for k in range(pm.LFILTER_BUFFERS):
            xd = dev(rt, x[k])
            yd = rt.torch.empty_like(xd)
            rt.hip.check(rt.lib.rcfm_lfilter_fir(C, n, taps_p, ntaps, rt.hip.ptr(state) if ntaps > 1 else None,
                                                 rt.hip.ptr(xd), rt.hip.ptr(yd), rt.hip.stream()))
            got.append(host(rt, yd))
        # float64 lfilter over the concatenation: what three buffers with a carried state must add up to
        ref_y, ref_z = pm.ref_lfilter(b, np.concatenate(list(x), axis=1), zi)
        ey = pm.worst_row(np.concatenate(got, axis=1), ref_y)
        ez = pm.worst_row(host(rt, state), ref_z) if ntaps > 1 else 0.0
        print("lfilter %d taps n=%d C=%d: y %.3g (bound %.3g) state %.3g (bound %.3g)" % (ntaps, n, C, ey, by, ez, bz))
        worst_y, worst_z = max(worst_y, ey), max(worst_z, ez)
    assert worst_y <= by and worst_z <= bz, (worst_y, worst_z)


def test_lfilter_in_place_is_refused(rt):
    """k_fir's workgroups need the inputs before their tile while others write outputs there, and k_fir_state reads x after
    y is complete: y == x cannot give lfilter's result, so the call is refused on the host and nothing is touched."""
    b = pm.filter_taps("random", 51, seed=3)
    taps, taps_p = rt.hip.float_array(b)
    x, zi = pm.lfilter_input(3, 4800, 51, 1, 4)
    xd, state = dev(rt, x[0]), dev(rt, zi)
    st = rt.lib.rcfm_lfilter_fir(3, 4800, taps_p, 51, rt.hip.ptr(state), rt.hip.ptr(xd), rt.hip.ptr(xd), rt.hip.stream())
    assert st == ERR_ARG and b"in place" in rt.lib.rcfm_last_error()
    assert np.array_equal(host(rt, xd), x[0]) and np.array_equal(host(rt, state), zi)
    # any overlap of [x, x + C n) and [y, y + C n), from either side; arrays that merely touch are fine
    flat = dev(rt, np.concatenate([x[0].reshape(-1), np.zeros(3 * 4800, np.float32)]))
    for xo, yo in ((0, 1), (1, 0), (0, 3 * 4800 - 1), (3 * 4800 - 1, 0)):
        st = rt.lib.rcfm_lfilter_fir(3, 4800, taps_p, 51, rt.hip.ptr(state), rt.hip.ptr(flat[xo:]), rt.hip.ptr(flat[yo:]),
                                     rt.hip.stream())
        assert st == ERR_ARG, (xo, yo)
    rt.hip.check(rt.lib.rcfm_lfilter_fir(3, 4800, taps_p, 51, rt.hip.ptr(state), rt.hip.ptr(flat), rt.hip.ptr(flat[3 * 4800:]),
                                         rt.hip.stream()))
    bound = pm.gpu_bound(pm.YARDSTICK["lfilter"])
    assert pm.worst_row(host(rt, flat[3 * 4800:]).reshape(3, 4800), pm.ref_lfilter(b, x[0], zi)[0]) <= bound


# ---- rcfm_hilbert ----------------------------------------------------------------------------------------------------------

def hilbert(rt, x):
    C, n = x.shape
    xd = dev(rt, x)
    zd = rt.torch.empty((C, n), dtype=rt.torch.complex64, device="cuda")
    rt.hip.check(rt.lib.rcfm_hilbert(C, n, rt.hip.ptr(xd), rt.hip.ptr(zd), rt.hip.stream()))
    return host(rt, zd)


def hilbert_sizes(rt):
    """(n, route): the listed lengths with the route asserted from the plan, plus the smallest n >= 16 of each route."""
    out = []
    for n in pm.HILBERT_ENGINE_SIZES:
        assert engine_row_length(rt, n) is not None, n
        out.append((n, "engine"))
    for n in pm.HILBERT_ROCFFT_SIZES:
        assert engine_row_length(rt, n) is None, n
        out.append((n, "rocfft"))
    assert pm.HILBERT_ROCFFT_SIZES[0] % 2 == 1 and all(pm.HILBERT_ROCFFT_SIZES[1] % p for p in range(2, 101))
    smallest = (next(n for n in range(16, 4096) if engine_row_length(rt, n) is not None),
                next(n for n in range(16, 4096) if engine_row_length(rt, n) is None))
    assert smallest == pm.HILBERT_SMALLEST, smallest        # the sizes the CPU yardstick was taken at
    assert os.environ.get("RCFM_FFT") != "rocfft"
    return out + [(smallest[0], "engine"), (smallest[1], "rocfft")]


def test_hilbert_both_routes_and_batches(rt):
    bound = pm.gpu_bound(pm.YARDSTICK["hilbert"])
    worst = 0.0
    for n, route in hilbert_sizes(rt):
        for C in pm.HILBERT_BATCHES:
            x = pm.spectral_input(C, n, n, False, 5)
            z = hilbert(rt, x)
            ez = pm.worst_row(z, pm.ref_hilbert(x))
            ex = pm.worst_row(z.real, x.astype(np.float64))
            print("hilbert %d (%s) C=%d: z %.3g Re z - x %.3g (bound %.3g)" % (n, route, C, ez, ex, bound))
            worst = max(worst, ez, ex)
    assert worst <= bound, worst


def test_hilbert_plan_cache_evicts_and_rebuilds_bit_identically(rt):
    """16 entries, least recently used out first: 18 more (n, C) pairs on the stream push the first one out; run again it
    is planned anew and returns the bits it returned the first time."""
    pairs = [(6000, 2)] + [(512 * k, 1 + k % 3) for k in range(1, 10)] + [(1000 + 7 * k, 1 + k % 2) for k in range(9)]
    assert len(set(pairs)) >= 18
    bound = pm.gpu_bound(pm.YARDSTICK["hilbert"])
    first = None
    x0 = pm.spectral_input(2, 6000, 6000, False, 9)
    for n, C in pairs:
        x = x0 if (n, C) == pairs[0] else pm.spectral_input(C, n, n, False, 9)
        z = hilbert(rt, x)
        assert pm.worst_row(z, pm.ref_hilbert(x)) <= bound, (n, C)
        if first is None:
            first = z
    again = hilbert(rt, x0)
    assert np.array_equal(again.view(np.float32), first.view(np.float32))


# ---- rcfm_pll_phase --------------------------------------------------------------------------------------------------------

def pll(rt, z, mult, want_imag):
    zd = dev(rt, z)
    od = rt.torch.empty(len(z), dtype=rt.torch.float32, device="cuda")
    rt.hip.check(rt.lib.rcfm_pll_phase(rt.hip.ptr(zd), len(z), float(mult), want_imag, rt.hip.ptr(od), rt.hip.stream()))
    return host(rt, od)


@pytest.mark.parametrize("mult", pm.PLL_INTEGER + pm.PLL_PRINCIPAL)
def test_pll_phase_inside_the_float32_range(rt, mult):
    """Magnitudes over primitives_model.pll_magnitude_range(mult): |z|^|mult| within 2^+-100.  Absolute error."""
    bound = pm.pll_gpu_bound(mult)
    worst = 0.0
    for count in pm.PLL_COUNTS:
        z = pm.pll_input(count, mult, 7)
        for want_imag in (0, 1):
            got = pll(rt, z, mult, want_imag)
            assert np.all(np.isfinite(got))
            worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - pm.ref_pll(z, mult, want_imag)))))
    report("pll_phase mult %g (absolute)" % mult, worst, bound)
    assert worst <= bound


@pytest.mark.parametrize("mult", [m for m in pm.PLL_INTEGER + pm.PLL_PRINCIPAL if abs(m) >= 2.5])
def test_pll_phase_outside_the_float32_range(rt, mult):
    """|z|^mult beyond 2^+-200, with |z| itself an ordinary float32.  numpy's complex64 power (the oracle's PLL.real /
    image) is NaN everywhere.  Multiply-out branch: the same pattern.  Principal branch: the kernel never forms the
    power and every output is finite."""
    for outside in (1, -1):
        z = pm.pll_input(4099, mult, 7, outside)
        assert np.all(np.isfinite(z.view(np.float32))) and np.all(np.abs(z) > 0)
        for want_imag in (0, 1):
            got, want = pll(rt, z, mult, want_imag), pm.f32_pll(z, mult, want_imag)
            assert np.all(np.isnan(want))
            if mult in pm.PLL_INTEGER:
                assert np.array_equal(np.isnan(got), np.isnan(want)), (mult, outside, np.isnan(got).mean())
            else:
                assert np.all(np.isfinite(got)) and np.all(np.abs(got) <= 1.0)


@pytest.mark.parametrize("mult", pm.PLL_INTEGER + pm.PLL_PRINCIPAL)
def test_pll_phase_of_zero(rt, mult):
    """NaN on both branches, as numpy's 0 / 0 -- but for mult = 0, where numpy's power is 1 whatever the base."""
    z = np.zeros(257, np.complex64)
    z[1::2] = pm.pll_input(128, mult, 3)
    for want_imag in (0, 1):
        got, want = pll(rt, z, mult, want_imag), pm.f32_pll(z, mult, want_imag)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.all(np.isfinite(got[1::2]))
        if mult == 0:
            assert np.all(got[0::2] == (0.0 if want_imag else 1.0))
        else:
            assert np.all(np.isnan(got[0::2]))


# ---- rcfm_discriminator ----------------------------------------------------------------------------------------------------

def discriminator(rt, iq):
    C, n = iq.shape
    xd = dev(rt, iq)
    dd = rt.torch.full((C, n), 7.0, dtype=rt.torch.float32, device="cuda")
    rt.hip.check(rt.lib.rcfm_discriminator(C, n, rt.hip.ptr(xd), rt.hip.ptr(dd), rt.hip.stream()))
    return host(rt, dd)


@pytest.mark.parametrize("C", pm.DISC_BATCHES)
def test_discriminator_rows_start_at_zero_and_scale_away(rt, C):
    bound = pm.gpu_bound(pm.YARDSTICK["discriminator"])
    worst = 0.0
    for n in pm.DISC_SIZES:
        iq = pm.discriminator_input(C, n, 6)
        ref = pm.ref_discriminator(iq)
        for scale in (1.0,) + pm.DISC_SCALES:
            scaled = (iq.astype(np.complex128) * scale).astype(np.complex64)
            d = discriminator(rt, scaled)
            assert np.all(d[:, 0] == 0.0), d[:, 0]                    # exactly, for EVERY row
            if n > 1:
                # against the steps of the scaled float32 samples, and against the unscaled ones': scale-free
                e = max(pm.worst_row(d, pm.ref_discriminator(scaled)), pm.worst_row(d, ref))
            else:
                e = 0.0
            worst = max(worst, report("discriminator n=%d C=%d x%g" % (n, C, scale), e, bound))
    assert worst <= bound


# ---- argument limits: refused on the host, nothing is launched --------------------------------------------------------------

def test_calls_over_the_launch_limits_are_refused_on_the_host(rt):
    lib, hip = rt.lib, rt.hip
    buf = rt.torch.zeros(1 << 16, dtype=rt.torch.float32, device="cuda")
    p, s = hip.ptr(buf), hip.stream()
    one, one_p = hip.float_array(np.ones(1))
    big = 65536                                                  # one more than a grid's y / z extent
    h = ctypes.c_void_p()
    assert lib.rcfm_resampler_create(big, 256, 256, 1, ctypes.byref(h)) == ERR_ARG and not h.value
    assert lib.rcfm_resampler_create(big, 250, 100, 0, ctypes.byref(h)) == ERR_ARG and not h.value
    assert lib.rcfm_filtfilt(big, 16, one_p, 1, p, p, s) == ERR_ARG
    assert lib.rcfm_lfilter_fir(big, 16, one_p, 1, None, p, hip.ptr(buf[32768:]), s) == ERR_ARG
    assert lib.rcfm_hilbert(big, 16, p, p, s) == ERR_ARG
    assert lib.rcfm_discriminator(big, 16, p, p, s) == ERR_ARG
    assert b"65535" in lib.rcfm_last_error()
    for C, n in ((0, 16), (1, 0), (-1, 16)):
        assert lib.rcfm_discriminator(C, n, p, p, s) == ERR_ARG
    # taps: the largest count whose LDS fits is accepted (and computes), one more is refused
    for name, limit in (("filtfilt", 2867), ("lfilter", 5461)):
        for ntaps in (limit, limit + 1):
            b = pm.filter_taps("random", ntaps, seed=5)
            taps, taps_p = hip.float_array(b)
            n = 3 * ntaps + 1
            x = pm.noise_rows(2, n, 8)
            xd = dev(rt, x)
            yd = rt.torch.zeros_like(xd)
            if name == "filtfilt":
                st = lib.rcfm_filtfilt(2, n, taps_p, ntaps, hip.ptr(xd), hip.ptr(yd), s)
                ref, key = (pm.ref_filtfilt(b, x) if ntaps == limit else None), "filtfilt"
            else:
                zi = pm.noise_rows(2, ntaps - 1, 9)
                zd = dev(rt, zi)
                st = lib.rcfm_lfilter_fir(2, n, taps_p, ntaps, hip.ptr(zd), hip.ptr(xd), hip.ptr(yd), s)
                ref, key = (pm.ref_lfilter(b, x, zi)[0] if ntaps == limit else None), "lfilter"
            if ntaps > limit:
                assert st == ERR_ARG and str(limit).encode() in lib.rcfm_last_error(), (name, ntaps, st)
                assert not host(rt, yd).any()
            else:
                hip.check(st)
                # (this is about the launch at the limit; the yardsticks stop at 200 taps, so: the parity tolerance)
                bound = pm.TOL
                assert report("%s at %d taps" % (name, ntaps), pm.worst_row(host(rt, yd), ref), bound) <= bound
    assert lib.rcfm_pll_phase(p, ctypes.c_size_t(4294967041), 1.0, 0, p, s) == ERR_ARG
