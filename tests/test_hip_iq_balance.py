"""GPU: the IQ balance (rcfm_tuner_iq_estimate, rcfm_tuner_iq_correct, rcfm_tuner_set_iq_balance) against its definition
in include/rcfm.h, evaluated in float64 by tests/iqbal_model.py.

Shapes (iqbal_model.FIXTURES), the smallest at which each form of the kernels runs:
  odd     n = 90 001     odd n: both sides of a pair in 16-byte loads; rocFFT; general gather form
  even    n = 600 000    even n: bin n / 2 is its own mirror, the descending side in 8-byte loads
  fast    n = 4 000 000  12 500- and 240 000-sample channels: fast gather form, real halos (120 016 bins); 123 segments
  nohalo  n = 100 000    one channel as wide as the band: the handle keeps no halos
  rocfft  n = 10 007     prime: the forward transform is rocFFT's, the halos are its two copies
Correction: the spectrum X is read back from an attached slot, corrected in place by the library, and compared bin for bin
with the float64 model applied to that same X: |got - exp| <= 6 2^-24 (|X[k]| + |beta| |X[k']|) -- three roundings per
component, sqrt(2) for two components, rounded up.  Estimate: |dP| <= 1e-9 sum |X[m]| |X[n - m]|, |dQ| <= 1e-9 Q (any
summation order of at most 2 10^6 pairs stays within pairs 2^-53 = 2.2e-10), and beta is the float32 rounding of the
model's finish on the device's own sums.  End to end: levels() of an auto-balanced load_raw within the project's levels
bound, 1e-4 of the strongest, of the float64 chain (numpy FFT, estimate, correct, notch, levels).
"""

import ctypes
import importlib.util
import os

import numpy as np
import pytest

import iqbal_model as model
import squelch_model
from conftest import ROOT, TOL, have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

CHANNELS = {
    "odd": [(50e6, 30000), (50.02e6, 20001)],
    "even": [(100e6, 240000), (100e6 + 240000, 240000)] + [(100e6 + 366250 + 12500 * i, 12500) for i in range(8)],
    "fast": [(100e6 + off, bw) for off, bw in model.E2E_CHANNELS],
    "nohalo": [(100e6, 100000)],
    "rocfft": [(100e6, 5000)],
}
BETA = complex(np.float32(-0.0237), np.float32(-0.0268))      # a fixed beta near the receiver's (float32 values)


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
def oracle():
    import radiocore_oracle
    return radiocore_oracle


_inputs = {}


def _input(name):
    """complex128 [n]: the received buffer of a fixture, computed once."""
    if name not in _inputs:
        _inputs[name] = model.fixture(name)
    return _inputs[name]


def _tuner(rc, name, demod=None):
    n = model.FIXTURES[name][0]
    t = rc.Tuner()
    for f, bw in CHANNELS[name]:
        t.add_channel(f, bw, demod(bw) if demod else None)
    t.request_bandwidth(float(n))
    return t, n


def _nan_fill(t):
    import torch
    torch.view_as_real(t).fill_(float("nan"))


class _Loaded:
    """A tuner whose spectrum lives in an attached slot the test can read: X0 is the device's own X after a plain load."""

    def __init__(self, rc, hip, name):
        self.hip, self.name = hip, name
        self.tuner, self.n = _tuner(rc, name)
        self.slot = self.tuner.spectrum_slot(self.n)
        self.halo = self.slot.rcfm_halo
        _nan_fill(self.slot)
        self.tuner.attach(self.slot, self.n)
        self.tuner.load(_input(name).astype(np.complex64))
        hip.torch().cuda.synchronize()
        self.X0 = self.slot.clone()
        self.handle = self.tuner._ready()

    def storage(self):
        return self.slot.cpu().numpy()

    def restore(self, nan_halos=True):
        """X back in the slot; the halos NaN, so that whoever leaves them untouched shows."""
        self.slot.copy_(self.X0)
        if nan_halos and self.halo:
            _nan_fill(self.slot[:self.halo])
            _nan_fill(self.slot[self.halo + self.n:])


_loaded = {}


@pytest.fixture()
def loaded(rc, hip):
    def get(name):
        if name not in _loaded:
            _loaded[name] = _Loaded(rc, hip, name)
        return _loaded[name]
    yield get


def _engine(hip, n):
    """True where the forward transform of length n runs on the engine (rcfm_fft_describe accepts it)."""
    plan = hip.FftPlan()
    return hip.lib().rcfm_fft_describe(n, 0, ctypes.byref(plan)) == 0


def test_the_shapes_take_the_forms_they_are_here_for(loaded, hip):
    forms = {}
    for name in sorted(model.FIXTURES):
        d = loaded(name)
        forms[name] = ("engine" if _engine(hip, d.n) else "rocfft", d.halo)
        print("%s: n = %d, halo %d, forward %s, %d pairs in %d segments" % (
            name, d.n, d.halo, forms[name][0], model.last_pair(d.n), _segments(hip, model.last_pair(d.n))))
        st = d.X0.cpu().numpy()
        assert not np.isnan(st.view(np.float32)).any()
        assert np.array_equal(st, model.with_halos(st[d.halo:d.halo + d.n], d.halo))       # the load's own halos
    assert forms["rocfft"][0] == "rocfft" and forms["odd"][0] == "rocfft" and forms["rocfft"][1] > 0
    assert forms["fast"] == ("engine", 120016) and forms["even"][0] == "engine"
    assert forms["nohalo"][1] == 0 and forms["odd"][1] > 0 and forms["even"][1] > 0


def _segments(hip, pairs):
    return int(min(hip.RCFM_IQ_MAX_SEGS, max((pairs + hip.RCFM_IQ_SEG_PAIRS - 1) // hip.RCFM_IQ_SEG_PAIRS, 1)))


# ---- correction, elementwise ------------------------------------------------------------------------------------------

def _correct(d, beta, notch):
    t = d.hip.torch()
    b = t.tensor([beta.real, beta.imag], dtype=t.float32, device="cuda")
    d.hip.check(d.hip.lib().rcfm_tuner_iq_correct(d.handle, d.hip.ptr(b), notch, d.hip.stream()))
    t.cuda.synchronize()
    return d.storage()


@pytest.mark.parametrize("name,notch", [("odd", 0), ("odd", 3), ("even", 1), ("even", 300000), ("fast", 2), ("nohalo", 1),
                                        ("nohalo", 50000), ("rocfft", 1), ("rocfft", 5003)])
def test_correct_elementwise(loaded, name, notch):
    d = loaded(name)
    n, halo = d.n, d.halo
    X = d.X0.cpu().numpy()[halo:halo + n]
    d.restore()
    got = _correct(d, BETA, notch)
    Y = got[halo:halo + n]
    exp = model.correct(X, BETA, notch)
    bound = model.correct_bound(X, BETA)
    zeros = model.notch_bins(n, notch)
    assert np.all(Y[zeros].view(np.uint32) == 0), "notch bins are exact zeros"
    err = np.abs(Y.astype(np.complex128) - exp)
    keep = np.ones(n, bool)
    keep[zeros] = False
    worst = float(np.max(err[keep] / bound[keep]))
    print("%s notch %d: worst |got - exp| / bound = %.3f, max|got - exp| / max|X| = %.3g"
          % (name, notch, worst, float(err.max() / np.abs(X).max())))
    assert np.all(err <= bound), (name, notch, worst)
    # the halos, written on NaN: bit for bit the far ends
    assert not np.isnan(got.view(np.float32)).any()
    assert np.array_equal(got.view(np.uint32), model.with_halos(Y, halo).view(np.uint32))
    # the correction did something: bin k carried about |beta| |X[k']| of its mirror
    assert float(np.max(np.abs(Y - X))) > 0.5 * abs(BETA) * float(np.abs(X).max())


@pytest.mark.parametrize("name,notch", [("odd", 0), ("even", 2), ("fast", 1), ("nohalo", 0), ("rocfft", 2)])
def test_correct_with_beta_zero_changes_nothing_but_the_notch(loaded, name, notch):
    d = loaded(name)
    n, halo = d.n, d.halo
    X = d.X0.cpu().numpy()[halo:halo + n]
    d.restore()
    got = _correct(d, 0j, notch)
    exp = X.copy()
    exp[model.notch_bins(n, notch)] = 0
    assert np.array_equal(got.view(np.uint32), model.with_halos(exp, halo).view(np.uint32))


# ---- estimate ---------------------------------------------------------------------------------------------------------

def _estimate(d, m_lo, m_hi, want_sums=True, want_beta=True, stream=None):
    t = d.hip.torch()
    sums = t.full((3,), float("nan"), dtype=t.float64, device="cuda") if want_sums else None
    beta = t.full((2,), float("nan"), dtype=t.float32, device="cuda") if want_beta else None

    def call():
        d.hip.check(d.hip.lib().rcfm_tuner_iq_estimate(d.handle, m_lo, m_hi, d.hip.ptr(sums) if want_sums else None,
                                                       d.hip.ptr(beta) if want_beta else None, d.hip.stream()))
    if stream is None:
        call()
    else:
        stream.wait_stream(t.cuda.current_stream())
        with t.cuda.stream(stream):
            call()
    t.cuda.synchronize()
    return (sums.cpu().numpy() if want_sums else None), (beta.cpu().numpy() if want_beta else None)


def _ranges(hip, n):
    last = model.last_pair(n)
    r = [(1, last), (1, 1), (last, last), (2, last - 1), (2, 3), (3, 4)]
    if last > 3 * hip.RCFM_IQ_SEG_PAIRS:
        # several segments, an odd first pair: the segment boundaries fall inside the range, away from its ends
        r.append((5, 5 + 2 * hip.RCFM_IQ_SEG_PAIRS + 4321))
        r.append((last - 3 * hip.RCFM_IQ_SEG_PAIRS, last))
    return r


@pytest.mark.parametrize("name", sorted(model.FIXTURES))
def test_estimate_against_the_model(loaded, hip, name):
    d = loaded(name)
    d.restore(nan_halos=False)
    n, halo = d.n, d.halo
    X = d.X0.cpu().numpy()[halo:halo + n]
    second = hip.torch().cuda.Stream()
    true = model.receiver()[2]
    for m_lo, m_hi in _ranges(hip, n):
        sums, beta = _estimate(d, m_lo, m_hi)
        exp, cross = model.estimate_sums(X, m_lo, m_hi)
        dP = abs(complex(sums[0], sums[1]) - complex(exp[0], exp[1]))
        dQ = abs(sums[2] - exp[2])
        print("%s pairs [%d, %d] (%d segments): |dP| / cross = %.3g, |dQ| / Q = %.3g, beta = %r"
              % (name, m_lo, m_hi, _segments(hip, m_hi - m_lo + 1), dP / cross, dQ / exp[2], complex(beta[0], beta[1])))
        assert dP <= 1e-9 * cross and dQ <= 1e-9 * exp[2], (name, m_lo, m_hi, dP / cross, dQ / exp[2])
        want = model.finish_f32(sums)
        assert beta.dtype == np.float32 and (beta[0], beta[1]) == want, (name, m_lo, m_hi, beta, want)
        # bit-identical: again on a second stream, and with either output NULL
        s2, b2 = _estimate(d, m_lo, m_hi, stream=second)
        s3, _ = _estimate(d, m_lo, m_hi, want_beta=False)
        _, b4 = _estimate(d, m_lo, m_hi, want_sums=False)
        for s in (s2, s3):
            assert np.array_equal(s.view(np.uint64), sums.view(np.uint64)), (name, m_lo, m_hi)
        for b in (b2, b4):
            assert np.array_equal(b.view(np.uint32), beta.view(np.uint32)), (name, m_lo, m_hi)
        if (m_lo, m_hi) == (1, model.last_pair(n)):
            # the fixture's condition (tests/test_iqbal_model.py) holds for the device's estimate as well
            assert abs(complex(beta[0], beta[1]) - true) <= model.QUALITY * abs(true)


def test_python_iq_imbalance_maps_frequencies_to_pairs(loaded):
    d = loaded("odd")
    d.restore(nan_halos=False)
    beta, sums = d.tuner.iq_imbalance()
    s_full, b_full = _estimate(d, 1, model.last_pair(d.n))
    assert isinstance(beta, complex) and beta == complex(b_full[0], b_full[1]) and np.array_equal(sums, s_full)
    beta, sums = d.tuner.iq_imbalance(f_lo=8000.2, f_hi=30000)
    s_band, b_band = _estimate(d, 8000, 29999)
    assert beta == complex(b_band[0], b_band[1]) and np.array_equal(sums, s_band)
    from radiocore.tools import iq
    assert iq.balance_from([(beta, sums)]) == model.finish(sums)
    for bad in (dict(f_lo=0), dict(f_hi=45002), dict(f_lo=100, f_hi=100)):
        with pytest.raises(ValueError):
            d.tuner.iq_imbalance(**bad)


# ---- end to end -------------------------------------------------------------------------------------------------------

_e2e = {}


def _e2e_case(rc, oracle, fmt):
    """(raw, expected levels with balance, the beta of the model) for the end-to-end band as cu8 / cs16, computed once."""
    if fmt not in _e2e:
        x = _input("fast")
        raw = model.quantise_cu8(x) if fmt == "cu8" else model.quantise_cs16(x)
        xq = model.from_cu8(raw) if fmt == "cu8" else model.from_cs16(raw)
        Y, beta = model.balance(np.fft.fft(xq), notch=1)
        ref = oracle.Tuner()
        for f, bw in CHANNELS["fast"]:
            ref.add_channel(f, bw, None)
        ref.request_bandwidth(float(model.E2E_N))
        exp = np.array([squelch_model.level(oracle, Y, model.E2E_N, *ref._roll(i)) for i in range(len(CHANNELS["fast"]))])
        _e2e[fmt] = (raw, exp, beta)
    return _e2e[fmt]


@pytest.mark.parametrize("fmt", ["cu8", "cs16"])
def test_end_to_end_levels_and_squelch(rc, hip, oracle, fmt):
    raw, exp, beta = _e2e_case(rc, oracle, fmt)
    tuner, n = _tuner(rc, "fast")
    assert tuner.input_frequency == 100e6
    tuner.set_iq_balance("auto", dc_notch=1)
    tuner.load_raw(raw)
    got = tuner.levels()
    peak = float(exp.max())
    err = float(np.max(np.abs(got - exp))) / peak
    plain, _ = _tuner(rc, "fast")
    plain.load_raw(raw)
    raw_levels = plain.levels()
    err_plain = np.abs(raw_levels - exp) / peak
    strongest = int(np.argmax(exp))
    assert strongest == 1                      # the wide station at +1.2 MHz; channels come in mirrored pairs (2 i, 2 i + 1)
    mirror = strongest ^ 1
    print("%s: beta(model) = %r, balanced max|got - exp| / max(exp) = %.3g; unbalanced %.3g, in the strongest channel's mirror %.3g"
          % (fmt, beta, err, float(err_plain.max()), float(err_plain[mirror])))
    assert got.dtype == np.float32 and err <= TOL, (fmt, err)
    # what the feature does: without it the image of the strongest station stands in its mirror channel, 29 dB down
    assert float(err_plain.max()) > TOL
    assert 1.0e-3 <= float(err_plain[mirror]) <= 1.6e-3, float(err_plain[mirror])
    # squelch 6 dB over the floor: thresholds at least 3 dB from every expected level
    bws = np.array([bw for _, bw in CHANNELS["fast"]], np.float64)
    thr = (np.median(exp / bws) * bws * 10.0 ** 0.6).astype(np.float32)
    assert squelch_model.margin_db(exp, thr) >= 3.0
    want = squelch_model.open_mask(exp, thr)
    assert sorted(np.flatnonzero(want)) == [1, 2, 5, 8]           # the channels with a station

    def mask(levels):
        t = hip.torch()
        power, th = hip.to_device(levels, t.float32), hip.to_device(thr, t.float32)
        out = hip.empty((len(levels),), t.uint8)
        hip.check(hip.lib().rcfm_squelch(hip.ptr(power), hip.ptr(th), len(levels), 0, None, hip.ptr(out), hip.stream()))
        return hip.to_host(out).astype(bool)
    assert np.array_equal(mask(got), want)
    opened = mask(raw_levels)
    assert opened[3] and not want[3], "without the balance the image of the station in channel 2 opens channel 3"


def _spectrum_after(tuner, n, x, slot):
    tuner.attach(slot, n)
    tuner.load(x)
    return slot.cpu().numpy().copy()


def test_fixed_mode_with_the_estimated_beta_is_auto_mode(rc, hip):
    for name in ("fast", "odd"):
        tuner, n = _tuner(rc, name)
        x = _input(name).astype(np.complex64)
        slot = tuner.spectrum_slot(n)
        plain = _spectrum_after(tuner, n, x, slot)
        beta, _ = tuner.iq_imbalance()
        tuner.set_iq_balance(beta, dc_notch=2)
        _nan_fill(slot)
        fixed = _spectrum_after(tuner, n, x, slot)
        tuner.set_iq_balance("auto", dc_notch=2)
        _nan_fill(slot)
        auto = _spectrum_after(tuner, n, x, slot)
        assert np.array_equal(fixed.view(np.uint32), auto.view(np.uint32)), name
        assert not np.array_equal(plain.view(np.uint32), auto.view(np.uint32))
        tuner.set_iq_balance(None)
        _nan_fill(slot)
        assert np.array_equal(_spectrum_after(tuner, n, x, slot).view(np.uint32), plain.view(np.uint32)), name


# ---- lanes, the default path, refusals ----------------------------------------------------------------------------------

def _am_tuner(rc, n=600_000, C=6, B=25000, A=8000):
    t = rc.Tuner()
    for i in range(C):
        t.add_channel(118.0e6 + float(B) * i, B, rc.AM(B, A))
    t.request_bandwidth(float(n))
    return t


def _buffers():
    x = _input("even").astype(np.complex64)
    return [x, np.ascontiguousarray(x[::-1]), np.conj(x)]


def test_lanes_follow_the_setting_and_match_one_lane(rc):
    from radiocore.tools import Lanes
    bufs = _buffers()
    one = _am_tuner(rc)
    one.set_iq_balance("auto", dc_notch=1)
    want = []
    for x in bufs:
        one.load(x)
        want.append(one.run_all())
    base = _am_tuner(rc)
    base.set_iq_balance("auto", dc_notch=1)
    lanes = Lanes(base, depth=2)
    tickets = [lanes.submit(x) for x in bufs]
    for k, t in enumerate(tickets):
        assert np.array_equal(lanes.result(t).view(np.uint32), want[k].view(np.uint32)), k
    # ... and when the setting changes between submissions
    base.set_iq_balance(None)
    off = _am_tuner(rc)
    tickets = [lanes.submit(x) for x in bufs[:2]]
    for k, t in enumerate(tickets):
        off.load(bufs[k])
        ref = off.run_all()
        assert np.array_equal(lanes.result(t).view(np.uint32), ref.view(np.uint32)), k
        assert not np.array_equal(ref, want[k])


def test_default_path_is_untouched(rc):
    """Never set, or set and reset to None: run_all's audio is bit for bit that of a tuner that never touched the setting."""
    bufs = _buffers()[:2]
    never, reset = _am_tuner(rc), _am_tuner(rc)
    reset.set_iq_balance("auto", dc_notch=4)
    reset.load(bufs[0])
    balanced = reset.run_all()
    reset.set_iq_balance(None)
    for x in bufs:
        never.load(x)
        reset.load(x)
        a, b = never.run_all(), reset.run_all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(never.levels().view(np.uint32), reset.levels().view(np.uint32))
    never.load(bufs[0])
    assert not np.array_equal(never.run_all(), balanced)


def test_refusals_under_sharding_and_windows(rc):
    tuner, n = _tuner(rc, "fast")
    x = _input("fast").astype(np.complex64)
    tuner.shard(1, 1)                                  # the +1.2 MHz channel: the load keeps a window of rows
    tuner.load(x)                                      # fine without a balance mode
    with pytest.raises(RuntimeError):
        tuner.iq_imbalance()                           # ... but the mirror bins were not kept
    tuner.set_iq_balance("auto")
    with pytest.raises(RuntimeError):
        tuner.load(x)
    tuner.set_iq_balance(0.01 - 0.02j)
    with pytest.raises(RuntimeError):
        tuner.load(x)
    tuner.set_iq_balance(None)
    tuner.load(x)
    # an attached window, adopted: the mirror bins live on another rank
    win, _ = _tuner(rc, "fast")
    slot = win.window_slot(n, 1, 1)
    assert slot is not None
    slot.zero_()
    win.attach_window(slot, n)
    win.adopt(n, 1, 1)
    with pytest.raises(RuntimeError):
        win.iq_imbalance()


def test_rtl_image_reject_example():
    """examples/rtl_image_reject.py at a reduced size: with the balance only the planted channels open; without it the
    mirror channels of the strong stations open as well."""
    spec = importlib.util.spec_from_file_location("rtl_image_reject", os.path.join(ROOT, "examples", "rtl_image_reject.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    balanced, unbalanced, planted, ghosts = mod.run(channels=120, rate=4_000_000, seconds=2, stations=7)
    assert len(planted) == 1 and len(planted[0]) == 7
    for b, u, p, g in zip(balanced, unbalanced, planted, ghosts):
        assert sorted(b) == sorted(p)
        assert set(p) <= set(u) and g and set(g) <= set(u) and not set(g) & set(p)
