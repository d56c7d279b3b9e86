"""GPU: per-channel signal levels (rcfm_tuner_levels) and the device-side squelch (rcfm_squelch) against their
definition in include/rcfm.h, evaluated by tests/squelch_model.py from the oracle in float64 on the complex64 input.

Levels: max|got - exp| <= 1e-4 * max(exp) over ALL channels of a buffer (the project's TOL convention, of peak), and the
worst RELATIVE error over the channels within 60 dB of the strongest, asserted at ten times what was measured
(4.96e-7 measured, on the mixed-bandwidth tuner at N = 4 000 000, so 5e-6 here).
Squelch: the mask equals the model's for thresholds proven to lie >= 3 dB from every expected level; closed rows are
exact zeros, open rows bit-identical to the same call with squelch off.
"""

import ctypes

import numpy as np
import pytest

import am_model
import squelch_model
import workloads
from conftest import TOL, have_gpu
from test_hip_am import _Profile

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

REL_60DB = 5e-6      # ten times the measured worst relative error within 60 dB of the strongest channel, one digit, up


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def oracle():
    import radiocore_oracle
    return radiocore_oracle


def _pair(rc, oracle, N, chans, kinds=None, A=8000):
    """A Tuner and the oracle's over chans = [(centre, bandwidth)]; kinds[i] names the demodulator class (None: none)."""
    tuner, ref = rc.Tuner(), oracle.Tuner()
    for i, (f, bw) in enumerate(chans):
        k = kinds[i] if kinds else None
        tuner.add_channel(f, bw, getattr(rc, k)(bw, A) if k else None)
        ref.add_channel(f, bw, None)
    tuner.request_bandwidth(float(N))
    ref.request_bandwidth(float(N))
    assert tuner.input_frequency == ref.input_frequency
    return tuner, ref


def _load(tuner, ref, x):
    tuner.load(x)
    ref.load(x.astype(np.complex128))         # the expectation in float64 (numpy transforms complex64 in single precision)


def _check_levels(got, exp, what):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == exp.shape, (got.dtype, got.shape, exp.shape)
    peak = float(np.max(exp))
    err = float(np.max(np.abs(got - exp))) / peak
    near = exp >= peak * 1e-6
    rel = float(np.max(np.abs(got[near] - exp[near]) / exp[near]))
    print("%s: %d channels, max|got - exp| / max(exp) = %.3g, worst relative error of the %d within 60 dB = %.3g"
          % (what, exp.size, err, int(near.sum()), rel))
    assert err <= TOL, (what, err)
    assert rel <= REL_60DB, (what, rel)


def _noise_and_tones(N, chans, f_in, seed):
    """complex64 [N]: white noise plus one tone near each channel centre, levels 6 dB apart from channel to channel."""
    rng = np.random.default_rng(seed)
    x = 0.02 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    t = np.arange(N, dtype=np.float64) / N
    for i, (f, bw) in enumerate(chans):
        x += 0.5 ** (i % 6) * np.exp(2j * np.pi * (int(f - f_in) + bw // 7) * t)
    return x.astype(np.complex64)


# ---- levels against the model --------------------------------------------------------------------------------------

def test_levels_airband_760_channels(rc, oracle):
    """The airband buffer: 760 AM stations of 25 kHz in 20 MSPS, levels spread over 20 dB (and the Hann window on top);
    the fast form, four workgroups per channel.  Two calls are bit-identical."""
    N, B, C = 20_000_000, 25000, 760
    centres = workloads.channel_grid(C, B)
    tuner, ref = _pair(rc, oracle, N, [(f, B) for f in centres])
    x = am_model.wideband(N, ref.input_frequency, centres, B, [am_model.station(i, B, seed=31) for i in range(C)], seed=31)
    _load(tuner, ref, x)
    got = tuner.levels()
    _check_levels(got, squelch_model.levels(oracle, ref), "airband")
    assert np.array_equal(got, tuner.levels())


MIXED = [(100e6, 240000), (100e6 + 240000, 240000)] + [(100e6 + 366250 + 12500 * i, 12500) for i in range(8)]


@pytest.mark.parametrize("N", [4_000_000, 600_000])
def test_levels_mixed_bandwidths(rc, oracle, N):
    """240 000- and 12 500-sample channels in one call (30 and 2 workgroups per channel).  N = 4 000 000: the fast
    form; N = 600 000: a 240 kHz channel is wide against N (window argument 1.26 rad), the fast gather's
    preconditions fail and the general form runs (64-bit modulo indexing, library cosine)."""
    tuner, ref = _pair(rc, oracle, N, MIXED)
    _load(tuner, ref, _noise_and_tones(N, MIXED, ref.input_frequency, seed=N % 97))
    got = tuner.levels()
    _check_levels(got, squelch_model.levels(oracle, ref), "mixed N=%d" % N)
    assert np.array_equal(got, tuner.levels())


@pytest.mark.parametrize("N", [90001, 900001])
def test_levels_odd_geometry(rc, oracle, N):
    """The tuner_odd fixture's geometry (N = 90001: channels of 30 000 and 20 001 samples, general form, odd N puts
    pi / N into the window argument) and the same channels in N = 900 001 (fast form: odd B, both head parities)."""
    chans = [(50e6, 30000), (50.02e6, 20001)]
    tuner, ref = _pair(rc, oracle, N, chans)
    r = np.random.default_rng(3)
    x = (r.standard_normal(N) + 1j * r.standard_normal(N)).astype(np.complex64)
    _load(tuner, ref, x)
    _check_levels(tuner.levels(), squelch_model.levels(oracle, ref), "odd N=%d" % N)


def _am_grid(rc, oracle, N, C, B, A=8000, kind="AM"):
    centres = workloads.channel_grid(C, B)
    tuner, ref = _pair(rc, oracle, N, [(f, B) for f in centres], kinds=[kind] * C, A=A)
    return tuner, ref, centres


def test_levels_shard_window_and_attached_spectrum(rc, oracle):
    """After shard: the shard's range only.  Through an attached window + adopt, and on an attached spectrum slot.
    Readiness: RCFM_ERR_STATE before a load and outside the window, RCFM_ERR_INDEX for a bad range."""
    import torch
    from radiocore._internal import hip
    lib = hip.lib()
    N, B, C = 2_000_000, 25000, 64
    first, count = 40, 16          # clear of the band centre: their bins do not wrap around bin 0
    tuner, ref, centres = _am_grid(rc, oracle, N, C, B)
    x = am_model.wideband(N, ref.input_frequency, centres, B, [am_model.station(i, B, seed=8) for i in range(C)], seed=8)
    out = torch.empty(C, dtype=torch.float32, device="cuda")
    assert lib.rcfm_tuner_levels(tuner._device_tuner(N), 0, C, hip.ptr(out), hip.stream()) == -5       # before a load
    _load(tuner, ref, x)
    exp = squelch_model.levels(oracle, ref)
    whole = tuner.levels()
    _check_levels(whole, exp, "whole")
    h = tuner._handle.value
    assert lib.rcfm_tuner_levels(h, 0, C + 1, hip.ptr(out), hip.stream()) == -2
    assert lib.rcfm_tuner_levels(h, -1, 1, hip.ptr(out), hip.stream()) == -2
    assert lib.rcfm_tuner_levels(h, 0, C, None, hip.stream()) == -4
    hip.check(lib.rcfm_tuner_levels(h, 5, 0, hip.ptr(out), hip.stream()))                              # an empty range

    sharded, _, _ = _am_grid(rc, oracle, N, C, B)
    sharded.shard(first, count)
    sharded.load(x)
    got = sharded.levels()
    _check_levels(got, exp[first:first + count], "shard")
    # (a windowed load keeps only the rows the shard reads: channel 0 is then outside it)
    assert lib.rcfm_tuner_levels(sharded._handle.value, 0, 1, hip.ptr(out), hip.stream()) in (0, -5)

    # the owner's spectrum bins of the window travel into a window slot of another tuner
    win, _, _ = _am_grid(rc, oracle, N, C, B)
    win.shard(first, count)
    slot = win.window_slot(N, first, count)
    assert slot is not None, "these channels' window must fit a window slot"
    fb, nb = win.window(N, first, count)
    win.attach_window(slot, N)
    X = ctypes.c_void_p()
    hip.check(lib.rcfm_tuner_spectrum(h, ctypes.byref(X)))
    hip.check(lib.rcfm_memcpy_d2d(ctypes.c_void_p(slot.data_ptr() + 8 * slot.rcfm_halo), ctypes.c_void_p(X.value + 8 * fb),
                                  ctypes.c_size_t(8 * nb), hip.stream()))
    win.adopt(N, first, count)
    got = win.levels()
    _check_levels(got, exp[first:first + count], "window")
    assert np.array_equal(got, whole[first:first + count])            # the same bins, the same order of the sums
    assert lib.rcfm_tuner_levels(win._handle.value, first - 1, 2, hip.ptr(out), hip.stream()) == -5

    att, _, _ = _am_grid(rc, oracle, N, C, B)
    att.attach(att.spectrum_slot(N), N)
    att.load(x)
    _check_levels(att.levels(), exp, "attached slot")


# ---- squelch -------------------------------------------------------------------------------------------------------

def _stations(kind, B, planted, buf=0):
    """{channel: complex [B]} of the planted stations: AM ones for AM / USB (USB hears the carrier offset as a tone), FM
    ones otherwise; levels spread over 20 dB."""
    if kind in ("AM", "USB"):
        return {i: am_model.station(i + 7 * buf, B, seed=5) for i in planted}
    stereo = kind == "WBFM"
    return {i: 10.0 ** (-(i % 5) / 4.0) * workloads.station_iq(i + buf, B, deviation=None if stereo else 0.2 * B, stereo=stereo)
            for i in planted}


def _thresholds(rc, oracle, ref, B, planted, C, db=10.0):
    """Thresholds 10 dB over the floor from the MODEL's levels, proven to lie >= 3 dB from every expected level and to
    open exactly the planted channels."""
    exp = squelch_model.levels(oracle, ref)
    thr = rc.tools.threshold_over_floor(exp, B, db)
    margin = squelch_model.margin_db(exp, thr)
    print("thresholds %.0f dB over the floor: nearest expected level %.1f dB away" % (db, margin))
    assert margin >= 3.0, margin
    want = squelch_model.open_mask(exp, thr)
    assert sorted(np.flatnonzero(want)) == sorted(planted)
    return thr, want


def _check_squelched(got, base, mask, what):
    got, base = np.asarray(got), np.asarray(base)
    assert got.shape == base.shape
    for i, is_open in enumerate(mask):
        if is_open:
            assert np.array_equal(got[i], base[i]), (what, "open row changed", i)
        else:
            assert not got[i].any(), (what, "closed row is not zero", i)        # (-0.0 and NaN would count as set)
            assert np.array_equal(got[i].view(np.uint32), np.zeros_like(got[i], np.uint32)), (what, i)


@pytest.mark.parametrize("kind,A", [("AM", 8000), ("USB", 8000), ("FM", 8000), ("AM", 7875)])
def test_run_all_stateless_kinds(rc, oracle, kind, A):
    """AM, USB, FM; A = 7875 gives rows of 31 500 bytes, unaligned for every odd channel: the 4-byte store path.
    The stage profile: squelch off launches neither stage, squelch on launches each once per rcfm_pipeline_run."""
    N, B, C = 2_000_000, 25000, 64
    planted = [0, 3, 10, 11, 30, 47, 63]
    tuner, ref, centres = _am_grid(rc, oracle, N, C, B, A=A, kind=kind)
    x = squelch_model.sparse_band(N, ref.input_frequency, centres, B, _stations(kind, B, planted), seed=2)
    _load(tuner, ref, x)
    thr, want = _thresholds(rc, oracle, ref, B, planted, C)
    with _Profile() as ran:
        base = tuner.run_all()
    assert ran["levels"] == 0 and ran["squelch"] == 0, ran
    with pytest.raises(RuntimeError):
        tuner.open_mask()
    tuner.set_squelch(thr)
    with _Profile() as ran:
        got = tuner.run_all()
    assert ran["levels"] == 1 and ran["squelch"] == 1, ran
    mask = tuner.open_mask()
    assert mask.dtype == bool and np.array_equal(mask, want)
    assert all(np.abs(base[i]).max() > 1e-3 for i in range(C)), "every channel carries audio without squelch"
    _check_squelched(got, base, want, kind)
    # a scalar threshold, NaN thresholds, and off again
    tuner.set_squelch(float(np.median(thr)))
    tuner.run_all()
    assert np.array_equal(tuner.open_mask(), want)
    nan_thr = thr.copy()
    nan_thr[[3, 30]] = np.nan
    tuner.set_squelch(nan_thr)
    got = tuner.run_all()
    closed = want.copy()
    closed[[3, 30]] = False
    assert np.array_equal(tuner.open_mask(), closed)
    _check_squelched(got, base, closed, kind + " NaN")
    tuner.set_squelch(None)
    with _Profile() as ran:
        assert np.array_equal(tuner.run_all(), base)
    assert ran["levels"] == 0 and ran["squelch"] == 0, ran
    with pytest.raises(ValueError):
        tuner.set_squelch(np.ones(C + 1))


@pytest.mark.parametrize("kind,N,B,A,C", [("MFM", 1_000_000, 25000, 8000, 24), ("WBFM", 1_200_000, 60000, 12000, 12)])
def test_state_carries_through_closed_buffers(rc, oracle, kind, N, B, A, C):
    """MFM / WBFM over two consecutive buffers: the squelch mutes after the demodulator chain, so the de-emphasis state
    advances as without it -- a channel closed in buffer 0 and open in buffer 1 carries exactly the audio the
    unsquelched tuner gives."""
    plain, ref, centres = _am_grid(rc, oracle, N, C, B, A=A, kind=kind)
    gated, _, _ = _am_grid(rc, oracle, N, C, B, A=A, kind=kind)
    sets = ([1, 4, C - 2], [1, 2, 5, C - 2])           # 2 and 5 open in the second buffer, 4 closes
    for buf, planted in enumerate(sets):
        x = squelch_model.sparse_band(N, ref.input_frequency, centres, B, _stations(kind, B, planted, buf), seed=buf)
        _load(plain, ref, x)
        gated.load(x)
        thr, want = _thresholds(rc, oracle, ref, B, planted, C)
        gated.set_squelch(thr)
        base = plain.run_all()
        got = gated.run_all()
        assert np.array_equal(gated.open_mask(), want)
        _check_squelched(got, base, want, (kind, buf))


def test_run_each_mixed_classes(rc, oracle):
    """Groups of AM, MFM and FM channels: levels and squelch launch once per rcfm_pipeline_run group, each on its part of
    the thresholds."""
    N, B, A, C = 1_000_000, 25000, 8000, 12
    kinds = ["AM"] * 3 + ["MFM"] * 3 + ["AM"] * 2 + ["FM"] * 2 + ["AM"] * 2
    planted = [1, 4, 7, 8, 11]
    centres = workloads.channel_grid(C, B)
    chans = [(f, B) for f in centres]
    plain, ref = _pair(rc, oracle, N, chans, kinds=kinds, A=A)
    gated, _ = _pair(rc, oracle, N, chans, kinds=kinds, A=A)
    st = {}
    for i in planted:
        st.update(_stations(kinds[i], B, [i]))
    x = squelch_model.sparse_band(N, ref.input_frequency, centres, B, st, seed=4)
    _load(plain, ref, x)
    gated.load(x)
    thr, want = _thresholds(rc, oracle, ref, B, planted, C)
    gated.set_squelch(thr)
    base = plain.run_each()
    with _Profile() as ran:
        got = gated.run_each()
    assert ran["levels"] == 5 and ran["squelch"] == 5, ran
    assert np.array_equal(gated.open_mask(), want)
    assert len(got) == C and all(g.shape == (A, 1) for g in got)
    _check_squelched(np.stack(got), np.stack(base), want, "run_each")


def test_lanes_depth_two(rc, oracle):
    """Lanes(depth=2) with squelch: audio and masks equal the one-lane loop's bit for bit, and the lanes' own levels of
    the buffers they hold are bit-identical to the one lane's."""
    import torch
    from radiocore.tools import Lanes
    N, B, A, C = 1_000_000, 25000, 8000, 24
    one, ref, centres = _am_grid(rc, oracle, N, C, B, A=A)
    sets = ([2, 9], [2, 3, 20], [0, 23], [9, 10, 11, 12])
    bufs = [squelch_model.sparse_band(N, ref.input_frequency, centres, B, _stations("AM", B, p, b), seed=b) for b, p in enumerate(sets)]
    ref.load(bufs[0].astype(np.complex128))
    thr = rc.tools.threshold_over_floor(squelch_model.levels(oracle, ref), B, 10.0)      # one calibration pass
    one.set_squelch(thr)
    want, masks, lv = [], [], []
    for b, x in enumerate(bufs):
        ref.load(x.astype(np.complex128))
        exp = squelch_model.levels(oracle, ref)
        assert squelch_model.margin_db(exp, thr) >= 3.0
        one.load(x)
        want.append(one.run_all())
        masks.append(one.open_mask())
        lv.append(one.levels())
        assert np.array_equal(masks[-1], squelch_model.open_mask(exp, thr)) and sorted(np.flatnonzero(masks[-1])) == sets[b]
    base, _, _ = _am_grid(rc, oracle, N, C, B, A=A)
    base.set_squelch(thr)
    lanes = Lanes(base, depth=2)
    tickets = [lanes.submit(x) for x in bufs]
    for i, t in enumerate(tickets):
        audio, mask = lanes.result(t, open_mask=True)
        assert np.array_equal(audio, want[i]), i
        assert np.array_equal(mask, masks[i]), i
    for k in range(2):          # lane k still holds buffer 2 + k
        with torch.cuda.stream(lanes._streams[k]):
            assert np.array_equal(lanes._tuners[k].levels(), lv[2 + k]), k
    base.set_squelch(None)
    t = lanes.submit(bufs[1])
    t2 = lanes.submit(bufs[1])
    audio, mask = lanes.result(t2, open_mask=True)      # the second lane follows the base tuner's setting
    assert mask is None and np.abs(audio[0]).max() > 1e-3
    assert isinstance(lanes.result(t), np.ndarray)


def test_entry_point_mask_only_and_fill_only():
    """rcfm_squelch with audio = NULL (mask only), with open = NULL, NaN on either side, rows of one float."""
    import torch
    from radiocore._internal import hip
    lib = hip.lib()
    power = np.array([1.0, 2.0, np.nan, 3.0, 0.0, 5.0], np.float32)
    thr = np.array([1.0, 2.5, 1.0, np.nan, 0.0, -1.0], np.float32)
    want = squelch_model.open_mask(power, thr)
    p, t = hip.to_device(power), hip.to_device(thr)
    mask = torch.full((6,), 7, dtype=torch.uint8, device="cuda")
    hip.check(lib.rcfm_squelch(hip.ptr(p), hip.ptr(t), 6, 12345, None, hip.ptr(mask), hip.stream()))
    assert mask.cpu().numpy().tolist() == [int(v) for v in want]
    for row in (1, 5000, 16384 + 4, 70001):
        audio = torch.full((6, row), 2.5, dtype=torch.float32, device="cuda")
        guard = audio.clone()
        hip.check(lib.rcfm_squelch(hip.ptr(p), hip.ptr(t), 6, row, hip.ptr(audio), None, hip.stream()))
        a = audio.cpu().numpy()
        _check_squelched(a, guard.cpu().numpy(), want, ("row", row))
    hip.check(lib.rcfm_squelch(hip.ptr(p), hip.ptr(t), 0, 8, None, None, hip.stream()))
    assert lib.rcfm_squelch(hip.ptr(p), hip.ptr(t), -1, 8, None, None, hip.stream()) == -4


def test_airband_squelch_example():
    """examples/airband_squelch.py at a reduced size: the channels it reports as open are the planted ones, and only
    they produce frames."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("airband_squelch", os.path.join(ROOT, "examples", "airband_squelch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opened, planted, msgs = mod.run(channels=120, rate=4_000_000, seconds=3, stations=7)
    assert len(planted) == 2 and all(len(p) == 7 for p in planted)
    assert [sorted(o) for o in opened] == [sorted(p) for p in planted]
    assert len(msgs) == 14
