"""GPU: the demodulator tails on signal content the rest of the suite never feeds them (tests/signal_edges.py).

Every other FM / MFM / WBFM parity input is a strong, clean, zero-mean station (workloads.station_iq): the clip of
mfm.py:65 / wbfm.py:100 never engages, the derived mean of the fused tails (kernels.hip k_fir51, lds_chain.hip) is ~0,
and the input's absolute scale is always O(1).  Here:

    clip      stations whose audio crosses ONE bound of the clip, both signs and an ordinary station in one band
    mean      stations whose discriminator averages +-0.4: the derived mean's DC-bin, tail and state terms are all large
    scale     the same band loaded at 2^k, k in {-24, -12, 0, +15} (weak bands .. raw int16 counts), every demodulator

on every route a tail can take -- the fused k_fir51<1> / <2>, the generic k_fir + k_dc_clip, the LDS chain with its
in-chain de-emphasis and with RCFM_OPT_LDS_DEEMPH off, the unfused chain -- each confirmed through the stage profile or by
reading the option back, through the batched run_all and, for one channel per band, the per-channel MFM / WBFM.run call.

The comparison target is signal_edges.Truth: the oracle with the float64 discriminator, fed with the oracle Tuner's
run_pruned (the reference's float32 unwrap is useless at these carrier offsets).  Bounds: 0.1 TOL for
HIP against the float64 truth and 0.05 TOL between two HIP evaluations of one result, as elsewhere in the suite.
tests/test_signal_edges.py pins the inputs' conditioning without a GPU.
"""

import ctypes

import numpy as np
import pytest

import am_model
import signal_edges as se
import ssb_model
import workloads
from conftest import TOL, have_gpu, rel_err
from test_hip_am import _Profile

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ROUNDING = 0.05 * TOL
CLIP32 = np.float32(0.999)
UNFUSED = dict(lds_chain=False, fused_tiles=False, phase_link=False)


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


def _ids(geometries):
    return ["%s-%d-%d" % (g[0], g[2], g[3]) for g in geometries]


# lds_chain.hip instantiates the in-chain de-emphasis for workgroups of up to 512 threads (lds_chain_deemph_supported):
# 12 000 -> 6000 runs the chain with more, so its de-emphasis is k_fir51 behind the chain whatever RCFM_OPT_LDS_DEEMPH says
NO_IN_CHAIN_DEEMPH = {(12000, 6000)}


def _routes(geometry):
    """(name, set_kernel_options arguments or None, RCFM_OPT_LDS_DEEMPH) of every route `geometry` is run on."""
    if geometry in se.LDS_ROWS:
        routes = [("lds_chain", None, 1), ("lds_chain, de-emphasis off chip", None, 0)]
        return routes + ([("unfused", UNFUSED, 1)] if geometry == se.LDS_ROWS[0] else [])
    if geometry in se.GENERIC:
        return [("generic fir + dc_clip", None, 1)]
    return [("fused fir51", None, 1), ("unfused", UNFUSED, 1)]


def _check_route(name, geometry, ran, options):
    """The stage profile of the last run_all (and the options read back) says the intended tail ran."""
    from radiocore._internal import hip
    ran = {k: v for k, v in ran.items() if v}
    print("   stages:", ran, "options:", options)
    if name == "fused fir51":
        assert ran.get("deemphasis", 0) > 0 and "dc_clip" not in ran and "lds_chain" not in ran, ran
    elif name == "generic fir + dc_clip":
        assert ran.get("deemphasis", 0) > 0 and ran.get("dc_clip", 0) > 0, ran
    elif name == "lds_chain":
        in_chain = (geometry[2], geometry[3]) not in NO_IN_CHAIN_DEEMPH
        assert ran.get("lds_chain", 0) > 0 and ("deemphasis" not in ran) == in_chain and "dc_clip" not in ran, ran
        assert options[hip.RCFM_OPT_LDS_DEEMPH] == 1
    elif name == "lds_chain, de-emphasis off chip":
        assert ran.get("lds_chain", 0) > 0 and ran.get("deemphasis", 0) > 0, ran
        assert options[hip.RCFM_OPT_LDS_DEEMPH] == 0
    else:
        assert "lds_chain" not in ran, ran
        assert [options[o] for o in (hip.RCFM_OPT_LDS_CHAIN, hip.RCFM_OPT_FUSED_TILES, hip.RCFM_OPT_PHASE_LINK)] == [0, 0, 0]


def _run_route(rc, geometry, bufs, kernel_options, lds_deemph):
    """The band's buffers through a fresh tuner: ([per buffer: audio [C, A, ch]], [per buffer: channel 0 through the
    per-channel call], stage profile of the last run_all, {option: value read back})."""
    from radiocore._internal import hip
    lib = hip.lib()
    kind, N, B, A, C = geometry
    ch = 2 if kind == "WBFM" else 1
    tuner = rc.Tuner()
    for f in se.centres_of(B, C):
        tuner.add_channel(f, B, getattr(rc, kind)(B, A))
    tuner.request_bandwidth(float(N))
    if kernel_options is not None:
        tuner.set_kernel_options(**kernel_options)
    handle = tuner._batched_demod(*tuner._plan_uniform(), 0)
    if not lds_deemph:
        hip.check(lib.rcfm_demod_set_option(handle, hip.RCFM_OPT_LDS_DEEMPH, 0))
    single = getattr(rc, kind)(B, A)                 # its own state, fed with the device tuner's samples
    batched, alone, ran = [], [], {}
    for b, rec in enumerate(bufs):
        tuner.load(rec["x"])
        if b == len(bufs) - 1:
            with _Profile() as ran:
                audio = tuner.run_all()
        else:
            audio = tuner.run_all()
        assert audio.shape == (C, A, ch) and audio.dtype == np.float32
        batched.append(audio)
        alone.append(np.asarray(single.run(tuner.run(0))).reshape(A, ch))
    options = {}
    for o in (hip.RCFM_OPT_LDS_CHAIN, hip.RCFM_OPT_FUSED_TILES, hip.RCFM_OPT_PHASE_LINK, hip.RCFM_OPT_LDS_DEEMPH):
        v = ctypes.c_int()
        hip.check(lib.rcfm_demod_get_option(handle, o, ctypes.byref(v)))
        options[o] = v.value
    return batched, alone, ran, options


# ---- the clip on every tail ------------------------------------------------------------------------------------------

def _clip_checks(tag, got, truth, unclipped, sign):
    """One channel of one buffer: parity, and for a clipping station the bound itself, leg by leg."""
    err = rel_err(got, truth)
    assert err <= 0.1 * TOL, (tag, err)
    if not sign:
        return err
    for leg in range(got.shape[1]):
        g, un = got[:, leg], unclipped[:, leg]
        mine, other = (g, -g) if sign > 0 else (-g, g)
        assert np.max(mine) == CLIP32, (tag, leg, float(np.max(mine)))            # the bound, exactly
        assert np.max(other) < CLIP32, (tag, leg, float(np.max(other)))           # and only that one
        n_got = int(np.count_nonzero(mine == CLIP32))
        n_truth = int(np.count_nonzero(sign * un >= se.CLIP))
        slack = int(np.count_nonzero(np.abs(np.abs(un) - se.CLIP) <= 1e-5))        # capped by test_signal_edges.py
        assert n_truth > 0.01 * len(un), (tag, leg, n_truth)
        assert abs(n_got - n_truth) <= slack, (tag, leg, n_got, n_truth, slack)
    return err


@pytest.mark.parametrize("geometry", se.GEOMETRIES, ids=_ids(se.GEOMETRIES))
def test_clip_on_every_tail(rc, geometry):
    """np.clip(., -0.999, 0.999) exists four times on the device (k_fir51's fused tail, k_dc_clip, the LDS chain's
    fin(), the unfused chain through the first two): every one must hit float32(0.999) exactly where the truth clips, on
    the truth's side only, on both WBFM legs, as often as the truth does -- three consecutive buffers of other stations,
    so the carried state differs from buffer to buffer."""
    bufs = se.evaluate("clip", geometry)
    for name, kernel_options, lds_deemph in _routes(geometry):
        batched, alone, ran, options = _run_route(rc, geometry, bufs, kernel_options, lds_deemph)
        worst = 0.0
        for b, rec in enumerate(bufs):
            for i, sign in enumerate(rec["tags"]):
                worst = max(worst, _clip_checks((name, "run_all", b, i), batched[b][i], rec["truth"][i],
                                                rec["unclipped"][i], sign))
            worst = max(worst, _clip_checks((name, "per channel", b, 0), alone[b], rec["truth"][0],
                                            rec["unclipped"][0], rec["tags"][0]))
        print(geometry, name, "worst rel err vs float64 truth %.2e" % worst)
        _check_route(name, geometry, ran, options)


# ---- the derived mean under a large DC level -------------------------------------------------------------------------

def _mean_residual(a, truth):
    return abs(float(np.mean(np.asarray(a, np.float64))) - float(np.mean(truth)))


@pytest.mark.parametrize("geometry", se.GEOMETRIES, ids=_ids(se.GEOMETRIES))
def test_derived_mean_under_a_dc_level(rc, geometry):
    """The fused tails never sum the audio: the mean follows from A x the DC bin x sum(b), minus the last 50 inputs of
    each leg weighted by suffix sums of the taps, plus the carried-in state.  With zero-mean stations every one of those
    terms is ~0; with the discriminator at +-0.4 they are O(0.4 A), O(0.4 x 50) and O(0.4 x 50).  The statistic that
    isolates the mean is |mean64(audio) - mean64(truth)| per buffer and channel: averaging removes the per-sample
    rounding that hides a mean error in a max-norm.

    Bound: the larger of 8 x the worst residual of ref32 (the oracle's float32 tail -- lfilter, np.mean, clip as the
    reference computes them -- on the float64 discriminator's output) and 16 x 2^-24 x (|level| + peak): a handful of
    float32 roundings on sums of magnitude A |level|.  The test prints HIP's and ref32's worst residual and the bound
    for every route (ref32 alone, from the oracle, stays at a few 1e-8 on these bands, so the second term,
    6e-7 .. 7e-7, is the bound everywhere).  Measured on an MI355X: HIP 1.4e-8 .. 7.1e-8, ref32 2.1e-8 .. 5.0e-8
    (DESIGN.md section 3.3 has the table per route)."""
    bufs = se.evaluate("dc", geometry, with_ref32=True)
    C = geometry[4]
    level = max(abs(v) for v in se.DC_LEVELS)
    peak = max(float(np.max(np.abs(rec["truth"][i][50 if b == 0 else 0:]))) for b, rec in enumerate(bufs) for i in range(C))
    ref32 = max(_mean_residual(rec["ref32"][i], rec["truth"][i]) for rec in bufs for i in range(C))
    bound = max(8.0 * ref32, 16.0 * 2.0 ** -24 * (level + peak))
    for name, kernel_options, lds_deemph in _routes(geometry):
        batched, alone, ran, options = _run_route(rc, geometry, bufs, kernel_options, lds_deemph)
        worst_err, worst_mean, where = 0.0, 0.0, None
        for b, rec in enumerate(bufs):
            for i in list(range(C)) + [-1]:                     # -1: channel 0 through the per-channel call
                got, truth = (batched[b][i], rec["truth"][i]) if i >= 0 else (alone[b], rec["truth"][0])
                worst_err = max(worst_err, rel_err(got, truth))
                r = _mean_residual(got, truth)
                if r > worst_mean:
                    worst_mean, where = r, (b, i)
        print("mean residual", geometry, name, "HIP %.2e at %s  ref32 %.2e  bound %.2e  (rel err %.2e)"
              % (worst_mean, where, ref32, bound, worst_err))
        assert worst_err <= 0.1 * TOL, (name, worst_err)
        assert worst_mean <= bound, (name, worst_mean, where, bound)
        _check_route(name, geometry, ran, options)


# ---- the input's absolute scale ----------------------------------------------------------------------------------------

SCALES = (-24, -12, 0, 15)
GAINS = (1.0, 0.1, 0.6, 0.05, 0.8)        # station amplitudes relative to 0.3: the squelch has something to decide
SCALE_BANDS = {"FM": (1_200_000, 60000, 12000), "MFM": (1_200_000, 60000, 12000), "WBFM": (1_200_000, 60000, 12000),
               "AM": (1_000_000, 25000, 8000), "USB": (1_000_000, 12500, 8000)}


def _scale_band(kind):
    N, B, A = SCALE_BANDS[kind]
    C = len(GAINS)
    if kind == "AM":
        st = [am_model.station(i, B, seed=6, level=1.0) for i in range(C)]
    elif kind == "USB":
        st = [ssb_model.station(i, B, seed=6, level=1.0) for i in range(C)]
    else:
        st = [workloads.station_iq(89 + i, B, stereo=(kind == "WBFM")) for i in range(C)]
    f_in = se.oracle_tuner(B, C, N).input_frequency
    x = se.wideband_from(st, N, f_in, se.centres_of(B, C), B, gain=0.3 * np.asarray(GAINS), noise=1e-4)
    return x, N, B, A, C


def _scaled(x, k):
    return x * np.float32(2.0 ** k)          # a power of two: exact in complex64


def _fresh_tuner(rc, kind, N, B, A, C, link):
    tuner = rc.Tuner()
    for f in se.centres_of(B, C):
        tuner.add_channel(f, B, getattr(rc, kind)(B, A))
    tuner.request_bandwidth(float(N))
    tuner.set_kernel_options(phase_link=link)
    return tuner


@pytest.mark.parametrize("kind", list(SCALE_BANDS))
def test_input_scale_does_not_matter(rc, kind):
    """Receivers hand over raw ADC counts (int16 full scale is 2^15) or very weak bands, and the reference is scale-free
    (np.angle; AM divides by the carrier, SSB by the RMS).  The device path forms products of two samples when the
    phase link is off, floors atan2's denominator, compares powers in the squelch: the same band loaded at 2^k must
    give the k = 0 audio within the bound for two HIP evaluations of one result, the Tuner's samples and levels must
    scale by 2^k and 2^2k, and thresholds scaled by 2^2k must open the same channels."""
    x, N, B, A, C = _scale_band(kind)
    for link in (True, False):
        base = {}
        for k in (0,) + tuple(s for s in SCALES if s):
            tuner = _fresh_tuner(rc, kind, N, B, A, C, link)
            tuner.load(_scaled(x, k))
            lv = tuner.levels()
            if k == 0:
                order = np.sort(lv.astype(np.float64))
                threshold = float(np.sqrt(order[1] * order[2]))       # between the stations at 0.1 and at 0.6
                assert order[2] > 10.0 * order[1]
                base["open"] = lv > threshold
                assert 0 < base["open"].sum() < C
            tuner.set_squelch(np.float32(threshold) * np.float32(2.0 ** (2 * k)))
            muted = tuner.run_all()
            mask = tuner.open_mask()
            tuner.set_squelch(None)
            tuner.reset_states()
            audio = tuner.run_all()
            iq = np.stack([tuner.run(i) for i in range(C)])
            assert np.all(np.isfinite(audio)) and np.all(np.isfinite(iq)) and np.all(np.isfinite(lv))
            if k == 0:
                base.update(audio=audio, iq=iq, lv=lv)
                assert float(np.max(np.abs(audio))) > 1e-2
                continue
            want_iq = base["iq"] * np.float32(2.0 ** k)
            errs = [rel_err(audio[i], base["audio"][i]) for i in range(C)]
            iq_errs = [rel_err(iq[i], want_iq[i]) for i in range(C)]
            lv_err = float(np.max(np.abs(lv.astype(np.float64) / (base["lv"].astype(np.float64) * 4.0 ** k) - 1.0)))
            print(kind, "link" if link else "no link", "k %+d" % k, "audio %.2e  iq %.2e (bit-identical: %s)  levels %.2e"
                  % (max(errs), max(iq_errs), np.array_equal(iq, want_iq), lv_err), "open", mask.astype(int))
            assert max(errs) <= ROUNDING, (kind, link, k, errs)
            assert max(iq_errs) <= ROUNDING, (kind, link, k, iq_errs)
            assert lv_err <= 1e-6, (kind, link, k, lv_err)
            assert np.array_equal(mask, base["open"]), (kind, link, k, mask, base["open"])
            for i in range(C):
                if mask[i]:
                    assert rel_err(muted[i], base["audio"][i]) <= ROUNDING, (kind, link, k, i)
                else:
                    assert np.all(muted[i] == 0), (kind, link, k, i)


def test_amplitude_range_over_which_fm_parity_holds(rc):
    """Documents the usable amplitude range: the FM band at 2^k, k = -60 .. +60, against the oracle's
    audio of the unscaled band (np.angle is scale-free), phase link on and off.  Asserted: parity to TOL for
    -24 <= k <= 15 -- 2^-24 of full scale up to raw int16 counts.  Printed: the table, and the first k on either side at
    which parity is lost or a non-finite value appears.  Measured on an MI355X: parity holds over the whole sweep (9.3e-7
    with the phase link, 8.0e-7 without it, 3.4e-6 at k = -60 where the products of two samples are float32 denormals)."""
    import radiocore_oracle as oracle
    x, N, B, A, C = _scale_band("FM")
    ref = se.oracle_tuner(B, C, N, [oracle.FM(B, A) for _ in range(C)])
    ref.load(x)
    want = [ref.channels()[i].demodulator.run(ref.run_pruned(i)) for i in range(C)]
    ks = sorted(set(range(-60, 61, 6)) | {15})
    for link in (True, False):
        tuner = _fresh_tuner(rc, "FM", N, B, A, C, link)
        table = {}
        for k in ks:
            with np.errstate(all="ignore"):
                tuner.load(_scaled(x, k))
                audio = tuner.run_all()
                finite = bool(np.all(np.isfinite(audio)))
                err = max(rel_err(np.nan_to_num(audio[i], nan=np.inf, posinf=np.inf, neginf=np.inf), want[i])
                          for i in range(C)) if finite else float("inf")
            table[k] = (err, finite)
            print("FM", "link   " if link else "no link", "k %+3d  worst rel err %.2e  finite %s" % (k, err, finite))
        good = [k for k in ks if table[k][0] <= TOL]
        lost_below = max([k for k in ks if k < 0 and k not in good], default=None)
        lost_above = min([k for k in ks if k > 0 and k not in good], default=None)
        print("FM", "link" if link else "no link", "parity holds for k in [%s, %s]; first lost below: %s, above: %s"
              % (min(good), max(good), lost_below, lost_above))
        for k in ks:
            if -24 <= k <= 15:
                assert table[k][0] <= TOL, (link, k, table[k])
