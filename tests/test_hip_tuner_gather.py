"""GPU: rcfm_tuner_run form by form -- the fast gather, the general gather, the table gather in front of rocFFT -- and the
haloed spectrum they read, against the float64 reference of tests/tuner_model.py, through hip.lib() directly
(rcfm_tuner_create with rolls and bandwidths: the Python Tuner derives rolls from frequencies and cannot place a channel on a
band edge).

Every comparison is per channel (max|delta_c| / max|ref_c|, worst channel, all rolls of a bandwidth in one rcfm_tuner_run)
and is held to primitives_model.gpu_bound(): four times the error of the same arithmetic in float32 on the CPU
(tests/test_tuner_model.py pins that), never more than conftest.TOL.  The form of every case is computed by
tuner_model.gather_form from what the library reports (rcfm_tuner_spectrum_layout, rcfm_fft_describe), never assumed.

    gather      reference from the device's OWN complex64 spectrum (read back): the gather, the window and the inverse
                FFT, isolated from the forward transform; engine bands with 16- and with 8-line tiles
    whole path  reference from np.fft.fft of the input in float64; bound from YARDSTICK["tuner_run"] + YARDSTICK_FFT
    halos       on NaN-prefilled attached storage, bit for bit: X[-halo:0] == X[n - halo:n], X[n:n + halo] == X[0:halo],
                written by the engine's last pass, by the copies behind rocFFT, by a sharded load (held bins only) and by
                rcfm_tuner_adopt; halo <= n / 2 for every handle, none where the widest channel would need more

Bounds (every case prints its worst channel against them; no MI355X figures are recorded here yet):
    gather alone, every form    4 x 3.6e-7 = 1.44e-6
    whole path                  4 x (3.6e-7 + 3.4e-7) = 2.8e-6
"""
import ctypes
import os

import numpy as np
import pytest

import primitives_model as pm
import tuner_model as tm
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

BOUND_GATHER = pm.gpu_bound(tm.YARDSTICK["tuner_run"])
BOUND_WHOLE = pm.gpu_bound(tm.YARDSTICK["tuner_run"] + tm.YARDSTICK_FFT)
BIG_N = 1_200_000
TUNER_IDS = ["n%d-B%s" % (n, "_".join(map(str, bws))) for n, bws in tm.TUNERS]


@pytest.fixture(scope="module")
def rt():
    import torch
    from radiocore._internal import hip

    class RT:
        pass
    r = RT()
    r.torch, r.hip, r.lib = torch, hip, hip.lib()
    assert os.environ.get("RCFM_FFT") != "rocfft", "RCFM_FFT=rocfft takes every transform off the engine"
    return r


def report(what, err, bound):
    print("%-72s %.3g (bound %.3g)" % (what, err, bound))
    return err


def engine_plan(rt, n):
    """Pass lengths of the engine's plan for n, or None where rcfm_fft_describe refuses the length (rocFFT then)."""
    plan = rt.hip.FftPlan()
    if rt.lib.rcfm_fft_describe(n, 0, ctypes.byref(plan)) != 0:
        return None
    assert plan.n == n
    return [int(plan.passes[i].L) for i in range(plan.npass)]


class DeviceTuner:
    """One handle of the table: for every bandwidth of `bws`, the channels tuner_model.rolls(n, B), in that order."""

    def __init__(self, rt, n, bws):
        self.rt, self.n, self.bws = rt, n, tuple(bws)
        self.ranges, roll, bw = {}, [], []
        for B in self.bws:
            r = tm.rolls(n, B)
            self.ranges[B] = (len(roll), len(r))
            roll += list(r)
            bw += [B] * len(r)
        self.nch = len(roll)
        self.t = ctypes.c_void_p()
        rt.hip.check(rt.lib.rcfm_tuner_create(n, self.nch, (ctypes.c_int64 * self.nch)(*roll),
                                              (ctypes.c_int32 * self.nch)(*bw), ctypes.byref(self.t)))
        halo, nn = ctypes.c_int64(), ctypes.c_int64()
        rt.hip.check(rt.lib.rcfm_tuner_spectrum_layout(self.t, ctypes.byref(halo), ctypes.byref(nn)))
        assert nn.value == n
        self.halo = int(halo.value)
        self.storage = None

    def close(self):
        if self.t:
            self.rt.hip.check(self.rt.lib.rcfm_tuner_destroy(self.t))
            self.t = None

    def option(self, option, value):
        self.rt.hip.check(self.rt.lib.rcfm_tuner_set_option(self.t, option, value))

    def attach_nan_storage(self):
        """[halo | n | halo] of the caller's, every element NaN: an element nobody writes cannot pass by luck."""
        self.storage = self.rt.torch.full((self.n + 2 * self.halo,), complex(float("nan"), float("nan")),
                                          dtype=self.rt.torch.complex64, device="cuda")
        self.rt.hip.check(self.rt.lib.rcfm_tuner_attach_spectrum(self.t, self.rt.hip.ptr(self.storage), 0, 0))

    def load(self, x):
        self.x = self.rt.torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
        self.rt.hip.check(self.rt.lib.rcfm_tuner_load(self.t, self.rt.hip.ptr(self.x), self.rt.hip.stream()))

    def bins(self):
        """Bins [0, n) of the loaded spectrum as the device holds them (rcfm_tuner_spectrum + rcfm_memcpy_d2h)."""
        X = ctypes.c_void_p()
        self.rt.hip.check(self.rt.lib.rcfm_tuner_spectrum(self.t, ctypes.byref(X)))
        host = np.empty(self.n, np.complex64)
        self.rt.hip.check(self.rt.lib.rcfm_memcpy_d2h(host.ctypes.data_as(ctypes.c_void_p), X, host.nbytes, self.rt.hip.stream()))
        self.rt.hip.check(self.rt.lib.rcfm_stream_sync(self.rt.hip.stream()))
        return host

    def window(self, first, count):
        """rcfm_tuner_window: channels [first, first + count) read bins [first_bin, first_bin + nbins) modulo n."""
        fb, nb = ctypes.c_int64(), ctypes.c_int64()
        self.rt.hip.check(self.rt.lib.rcfm_tuner_window(self.t, first, count, ctypes.byref(fb), ctypes.byref(nb)))
        return int(fb.value), int(nb.value)

    def held_storage(self):
        """The attached storage on the host: [halo + n + halo]."""
        self.rt.torch.cuda.synchronize()
        return self.storage.cpu().numpy()

    def run(self, B, first=None, count=None):
        f0, c0 = self.ranges[B]
        first, count = f0 if first is None else first, c0 if count is None else count
        out = self.rt.torch.empty((count, B), dtype=self.rt.torch.complex64, device="cuda")
        self.rt.hip.check(self.rt.lib.rcfm_tuner_run(self.t, first, count, self.rt.hip.ptr(out), self.rt.hip.stream()))
        self.rt.torch.cuda.synchronize()
        return out.cpu().numpy()

    def form(self, B):
        rt = self.rt
        return (tm.gather_form(self.n, self.halo, B, engine_plan(rt, B) is not None, engine_plan(rt, self.n) is not None),
                tm.nyquist_mode(self.n, B))


@pytest.fixture(scope="module")
def loaded(rt):
    """idx -> (DeviceTuner of tm.TUNERS[idx] with noise(n) loaded into its own storage, the device's bins [0, n))."""
    cache = {}

    def get(idx):
        if idx not in cache:
            n, bws = tm.TUNERS[idx]
            d = DeviceTuner(rt, n, bws)
            d.load(tm.noise(n))
            cache[idx] = (d, d.bins())
        return cache[idx]
    yield get
    for d, _ in cache.values():
        d.close()


# ---- every route is reached ------------------------------------------------------------------------------------------------

def test_the_table_reaches_every_form_by_what_the_library_reports(rt):
    forms, producers = {}, set()
    for n, bws in tm.TUNERS:
        d = DeviceTuner(rt, n, bws)
        try:
            assert 2 * d.halo <= n and d.halo == tm.tuner_halo(n, bws), (n, bws, d.halo)
            for B in bws:
                forms[(n, bws, B)] = d.form(B)
                print("n=%d halo=%d B=%d: %s, nyquist %s" % ((n, d.halo, B) + forms[(n, bws, B)]))
            producers.add(("engine" if engine_plan(rt, n) else "rocfft", d.halo > 0))
        finally:
            d.close()
    reached = {(n % 2, f, m) for (n, _, _), (f, m) in forms.items()}
    for parity in (0, 1):
        assert {(parity, "fast", "down"), (parity, "fast", "none")} <= reached, reached
    assert {("general", "down"), ("general", "none"), ("tables", "down"), ("tables", "none")} <= set(forms.values())
    wide = [forms[k] for k in forms if k[2] == k[0]]
    assert len(wide) >= 2 and set(wide) == {("general", "none")} and any(k[2] == k[0] and k[0] % 2 == 0 for k in forms)
    assert forms[(10125, (1,), 1)] == ("tables", "none") and forms[(10125, (2,), 2)] == ("tables", "none")
    n0, bws0 = tm.TUNERS[0]                       # both sides of the series limit in one handle
    assert forms[(n0, bws0, 800)][0] == "fast" and forms[(n0, bws0, 810)][0] == "general"
    assert {("engine", True), ("rocfft", True), ("engine", False)} <= producers, producers
    assert any(f == "fast" and engine_plan(rt, n) is None for (n, _, _), (f, _) in forms.items())
    assert any(f == "general" and len(engine_plan(rt, B)) == 3 for (_, _, B), (f, _) in forms.items()), "no three-pass inverse"


# ---- the gather, isolated from the forward FFT -------------------------------------------------------------------------------

def run_cases(rt, d, ref_of, bound, label):
    """Every bandwidth of the handle, all rolls in one rcfm_tuner_run; engine bands with both tile widths."""
    worst = 0.0
    for B in d.bws:
        form, mode = d.form(B)
        ref = ref_of(B)
        for narrow in ((0, 2) if form != "tables" else (1,)):
            d.option(rt.hip.RCFM_TUNER_OPT_NARROW_TILES, narrow)
            err = tm.channel_errors(d.run(B), ref)
            worst = max(worst, report("%s n=%d B=%d %s/%s%s (worst roll %d)" %
                                      (label, d.n, B, form, mode, {0: " 16-line tiles", 2: " 8-line tiles", 1: ""}[narrow],
                                       tm.rolls(d.n, B)[int(np.argmax(err))]), float(err.max()), bound))
        d.option(rt.hip.RCFM_TUNER_OPT_NARROW_TILES, 1)
    return worst


@pytest.mark.parametrize("idx", range(len(tm.TUNERS)), ids=TUNER_IDS)
def test_gather_against_float64_of_the_devices_own_spectrum(rt, loaded, idx):
    d, X = loaded(idx)
    assert np.all(np.isfinite(X.view(np.float32)))
    assert run_cases(rt, d, lambda B: tm.ref_channels(X, d.n, B), BOUND_GATHER, "gather") <= BOUND_GATHER


def test_the_large_size_has_no_aligned_plan_and_the_option_changes_nothing(rt, loaded):
    """RCFM_TUNER_OPT_ALIGNED_PLAN at n = 1 200 000: what rcfm_tuner_create decides is restated from the described plan
    (three passes, beyond 256 MiB, a last pass that straddles lines) and seen in the spectrum: the same plan, the same bits."""
    idx = [n for n, _ in tm.TUNERS].index(BIG_N)
    d, X1 = loaded(idx)
    lengths = engine_plan(rt, BIG_N)
    found = len(lengths) == 3 and 8 * BIG_N > (256 << 20) and (lengths[0] * lengths[1]) % 16 != 0
    print("n=%d: passes %s, aligned plan %s" % (BIG_N, lengths, found))
    assert not found
    other = DeviceTuner(rt, *tm.TUNERS[idx])
    try:
        other.option(rt.hip.RCFM_TUNER_OPT_ALIGNED_PLAN, 0)
        other.load(tm.noise(BIG_N))
        X0 = other.bins()
        assert np.array_equal(X0.view(np.uint64), X1.view(np.uint64)) == (not found)
        assert run_cases(rt, other, lambda B: tm.ref_channels(X0, BIG_N, B), BOUND_GATHER, "aligned plan off") <= BOUND_GATHER
    finally:
        other.close()


# ---- whole path against float64 -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx", range(len(tm.TUNERS)), ids=TUNER_IDS)
def test_whole_path_against_float64_of_the_input(rt, loaded, idx):
    d, X = loaded(idx)
    X64 = tm.spectrum64(d.n)
    report("forward FFT n=%d (%s), of the spectrum's peak" % (d.n, "engine" if engine_plan(rt, d.n) else "rocfft"),
           float(np.max(np.abs(X - X64)) / np.max(np.abs(X64))), pm.gpu_bound(tm.YARDSTICK_FFT))
    assert run_cases(rt, d, lambda B: tm.ref_channels_of_input(d.n, B), BOUND_WHOLE, "whole path") <= BOUND_WHOLE


# ---- the halos ------------------------------------------------------------------------------------------------------------------

def same_bits(a, b):
    """Equal values (a NaN on either side fails) and equal bit patterns."""
    return bool(np.all(a == b)) and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_halos(d, held=None):
    """storage = [halo | n | halo]; held(bin) -> bool array: the bins a sharded load has stored (None: all)."""
    S, n, h = d.held_storage(), d.n, d.halo
    assert S.shape == (n + 2 * h,) and 2 * h <= n
    X = S[h:h + n]
    keep = np.ones(n, bool) if held is None else held(np.arange(n))
    assert np.all(np.isfinite(X[keep].view(np.float32))), "a held bin was never written"
    if h == 0:
        return 0
    left, right = keep[n - h:], keep[:h]
    assert same_bits(S[:h][left], X[n - h:][left]), "X[-halo:0] != X[n - halo:n]"
    assert same_bits(S[h + n:][right], X[:h][right]), "X[n:n + halo] != X[0:halo]"
    return int(left.sum()) + int(right.sum())


@pytest.mark.parametrize("idx", range(len(tm.TUNERS) + 1), ids=TUNER_IDS + ["halo-is-half-of-n"])
def test_halos_repeat_the_far_ends_bit_for_bit(rt, idx):
    """The engine's last pass (default plan) and the two copies behind rocFFT (n = 10007).  B == n: the widest channel
    would need more than n / 2 -- the handle keeps no halo, and halo == n / 2 exactly is the widest that does."""
    n, bws = (tm.TUNERS + (tm.HALO_EDGE,))[idx]
    d = DeviceTuner(rt, n, bws)
    try:
        print("n=%d B=%s: halo %d, forward %s" % (n, bws, d.halo, "engine" if engine_plan(rt, n) else "rocfft"))
        assert 2 * d.halo <= n, "halo > n / 2: a bin would belong to both halos"
        assert d.halo == tm.tuner_halo(n, bws)
        assert d.halo == 0 or d.halo >= max(bws) // 2 + 2
        d.attach_nan_storage()
        d.load(tm.noise(n))
        assert check_halos(d) == 2 * d.halo
        if idx < len(tm.TUNERS):          # the attached storage serves the channels like the handle's own
            B = bws[-1]
            assert report("from attached storage n=%d B=%d" % (n, B), tm.worst_channel(d.run(B), tm.ref_channels_of_input(n, B)),
                          BOUND_WHOLE) <= BOUND_WHOLE
    finally:
        d.close()


def test_halos_after_a_sharded_load_hold_the_windows_bins(rt):
    """rcfm_tuner_shard + load at n = 1 200 000: the last pass stores only the rows the shard's channels read; the channels
    with rolls 0, 3 and n - 5 read across bin 0, so both halos are needed and must hold what was stored."""
    idx = [n for n, _ in tm.TUNERS].index(BIG_N)
    n, bws = tm.TUNERS[idx]
    B = bws[0]
    assert tm.rolls(n, B)[:3] == (0, 3, n - 5)
    d = DeviceTuner(rt, n, bws)
    try:
        first, count = d.ranges[B][0], 3
        d.attach_nan_storage()
        rt.hip.check(rt.lib.rcfm_tuner_shard(d.t, first, count))
        fb, nb = d.window(first, count)
        print("shard window: first bin %d, %d bins of %d; halo %d" % (fb, nb, n, d.halo))
        assert B + 8 <= nb < n // 2 and (0 - fb) % n < nb, "the window must be a part of the spectrum around bin 0"
        d.load(tm.noise(n))
        checked = check_halos(d, lambda b: (b - fb) % n < nb)
        assert checked >= 2 * (B // 2 + 2)                       # at least what the channels read beyond either end
        got = d.run(B, first, count)
        assert report("sharded load n=%d B=%d, rolls 0, 3, n - 5" % (n, B),
                      tm.worst_channel(got, tm.ref_channels_of_input(n, B)[:3]), BOUND_WHOLE) <= BOUND_WHOLE
        assert rt.lib.rcfm_tuner_run(d.t, first + 3, 1, rt.hip.ptr(rt.torch.empty(B, dtype=rt.torch.complex64, device="cuda")),
                                     rt.hip.stream()) != 0       # a channel outside the shard is refused
    finally:
        d.close()


def test_halos_after_adopt(rt, loaded):
    """rcfm_tuner_adopt: the caller wrote bins [0, n) into the attached storage; adopt repeats the ends in the halos."""
    src, X = loaded(0)
    d = DeviceTuner(rt, *tm.TUNERS[0])
    try:
        assert d.halo > 0
        d.attach_nan_storage()
        d.storage[d.halo:d.halo + d.n] = rt.torch.from_numpy(X).to("cuda")
        rt.hip.check(rt.lib.rcfm_tuner_adopt(d.t, 0, d.nch, rt.hip.stream()))
        fb, nb = d.window(0, d.nch)                                # adopt refreshes the halos of the bins the range reads
        print("adopt: window first bin %d, %d bins of %d; halo %d" % (fb, nb, d.n, d.halo))
        checked = check_halos(d, lambda b: (b - fb) % d.n < nb)
        assert checked >= 2 * (max(d.bws) // 2 - 5)               # the widest channel at bases n - 3 and 5
        B = d.bws[0]
        assert np.array_equal(d.run(B), src.run(B))              # the same bins, the same kernel: the same bits
    finally:
        d.close()
