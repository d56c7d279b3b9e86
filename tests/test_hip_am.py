"""GPU: the AM demodulator (include/rcfm.h RCFM_AM) against its specification, built from the oracle's pieces
(tests/am_model.py): envelope |x|, radiocore_oracle.Decimate, division by the buffer's mean, minus 1, clip.

Every route a chunk can take (decimating tile, engine with a separate resample, rocFFT), the envelope link of
rcfm_pipeline_run and its complex fall-back, the two places where AM must not take the FM paths (the LDS-resident
chain, the phase link), batches, the Tuner's batched calls, graph replay and Lanes.

Tolerance: max|delta| <= 1e-4 * max|expected| (BASELINE.json north star), float32 end to end.
"""

import ctypes

import numpy as np
import pytest

import am_model
import workloads
from conftest import TOL, have_gpu, rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def oracle():
    import radiocore_oracle
    return radiocore_oracle


def _stages_run(lib, hip):
    """{stage name: launches} from librcfm's stage profile (rcfm_profile_*)."""
    out = {}
    for st in range(lib.rcfm_profile_stage_count()):
        ms, cnt = ctypes.c_double(), ctypes.c_int64()
        hip.check(lib.rcfm_profile_read(st, ctypes.byref(ms), ctypes.byref(cnt)))
        out[lib.rcfm_profile_stage_name(st).decode()] = int(cnt.value)
    return out


class _Profile:
    """with _Profile() as ran: ... -- ran holds the stage launches of the block afterwards."""

    def __enter__(self):
        from radiocore._internal import hip
        self.hip, self.lib = hip, hip.lib()
        self.hip.check(self.lib.rcfm_profile_reset())
        self.hip.check(self.lib.rcfm_profile_enable((1 << self.lib.rcfm_profile_stage_count()) - 1))
        self.ran = {}
        return self.ran

    def __exit__(self, *exc):
        try:
            self.ran.update(_stages_run(self.lib, self.hip))
        finally:
            self.hip.check(self.lib.rcfm_profile_enable(0))
        return False


def _set(demod, option, value):
    from radiocore._internal import hip
    hip.check(hip.lib().rcfm_demod_set_option(demod._handle.value, option, value))


# ---- one channel through each route --------------------------------------------------------------------------------

ROUTES = [
    # (B, A, options switched off, stages that must have launched, stages that must not)
    (25000, 8000, (), ("rfft_B", "ifft_A"), ("audio_spectrum",)),                   # decimating tile
    (25000, 8000, ("RCFM_OPT_DECIM_TILE",), ("rfft_B", "audio_spectrum", "ifft_A"), ()),   # engine, separate resample
    (25000, 8000, ("RCFM_OPT_FUSED_TILES",), ("rfft_B", "audio_spectrum", "ifft_A"), ()),
    (22000, 8000, (), ("rfft_B", "audio_spectrum", "ifft_A"), ()),                 # 2^4 5^3 11: rocFFT
    (25000, 7875, (), ("rfft_B", "audio_spectrum", "ifft_A"), ()),                 # odd A on the engine (75 x 105)
    (25000, 7999, (), ("rfft_B", "audio_spectrum", "ifft_A"), ()),                 # odd prime A: rocFFT
]


@pytest.mark.parametrize("B,A,off,want,never", ROUTES)
def test_single_channel_routes(rc, oracle, B, A, off, want, never):
    from radiocore._internal import hip
    x = am_model.am_iq(B, 0.6, tones=(440.0, 1330.0, 2900.0), amps=(1.0, 0.5, 0.3), offset=700, level=0.2,
                       noise=0.01, seed=3).astype(np.complex64)
    am = rc.AM(B, A)
    for o in off:
        _set(am, getattr(hip, o), 0)
    with _Profile() as ran:
        got = am.run(x)
    exp = am_model.expect(oracle, x, B, A)
    assert got.shape == (A, 1) and got.dtype == np.float32
    err = rel_err(got, exp)
    print(B, A, off, err, {k: v for k, v in ran.items() if v})
    assert err <= TOL
    assert ran["envelope"] == 1 and ran["am_tail"] == 1, ran
    for st in want:
        assert ran[st] >= 1, (st, ran)
    for st in never + ("discriminator", "deemphasis", "deemph_state", "dc_clip", "lds_chain", "pilot_stage"):
        assert ran[st] == 0, (st, ran)


@pytest.mark.parametrize("B,A", [(25000, 8000), (22000, 8000)])
def test_batch_equals_single_calls(rc, oracle, B, A):
    xs = np.stack([am_model.station(i, B, seed=4) for i in range(7)]).astype(np.complex64)
    got = rc.AM(B, A, batch=7).run(xs)
    assert got.shape == (7, A, 1)
    one = rc.AM(B, A)
    for i in range(7):
        single = one.run(xs[i])
        assert rel_err(got[i], single) <= TOL, i
        assert rel_err(got[i], am_model.expect(oracle, xs[i], B, A)) <= TOL, i


# ---- physics ---------------------------------------------------------------------------------------------------------

def _hamming_weight(B, f):
    """Decimate's frequency-domain periodic Hamming weight at f Hz of a B-point channel (W(0) = 1)."""
    return 0.54 + 0.46 * np.cos(2 * np.pi * f / B)


def test_tone_comes_out_at_the_modulation_index(rc):
    B, A, m = 25000, 8000, 0.5
    got = rc.AM(B, A).run(am_model.am_iq(B, m, tones=(1000.0,)).astype(np.complex64))[:, 0]
    # the decimator passes 1 kHz with its Hamming weight (0.9855 at B = 25 000); the AM chain adds nothing to it
    want = m * _hamming_weight(B, 1000.0) * np.sin(2 * np.pi * 1000.0 * np.arange(A) / A)
    assert np.max(np.abs(got - want)) <= 1e-3, np.max(np.abs(got - want))
    assert abs(np.max(got) - m) < 0.02


def test_overmodulation_hits_the_clip(rc, oracle):
    B, A = 25000, 8000
    x = am_model.am_iq(B, 1.2, tones=(700.0,)).astype(np.complex64)
    got = rc.AM(B, A).run(x)
    assert np.max(got) == np.float32(0.999) and np.min(got) >= np.float32(-0.999)
    assert np.count_nonzero(got == np.float32(0.999)) > 10
    assert rel_err(got, am_model.expect(oracle, x, B, A)) <= TOL


def test_level_does_not_matter(rc):
    B, A = 25000, 8000
    x = am_model.station(5, B, seed=1)
    am = rc.AM(B, A)
    ref = am.run(x.astype(np.complex64))
    for k in (1e-3, 1e3):
        got = am.run((x * k).astype(np.complex64))
        assert np.max(np.abs(got - ref)) <= 1e-5, (k, np.max(np.abs(got - ref)))


@pytest.mark.parametrize("offset", [-2000, 2000])
def test_carrier_offset_does_not_matter(rc, offset):
    B, A = 25000, 8000
    am = rc.AM(B, A)
    centred = am.run(am_model.am_iq(B, 0.7, tones=(600.0, 1800.0), amps=(1.0, 0.6)).astype(np.complex64))
    shifted = am.run(am_model.am_iq(B, 0.7, tones=(600.0, 1800.0), amps=(1.0, 0.6), offset=offset).astype(np.complex64))
    assert np.max(np.abs(shifted - centred)) <= 1e-5, np.max(np.abs(shifted - centred))


@pytest.mark.parametrize("B,A", [(25000, 8000), (22000, 8000), (25000, 7875)])
def test_silent_channel_gives_zeros(rc, B, A):
    got = rc.AM(B, A).run(np.zeros(B, np.complex64))
    assert not np.isnan(got).any() and np.all(got == 0)


# ---- the Tuner -----------------------------------------------------------------------------------------------------

def _am_band(rc, oracle, C, B, A, N, seed, raster=None, kinds=None, loud=()):
    """A tuner and the oracle's over C channels (AM unless kinds says otherwise) and a seeded band of AM stations
    (FM stations from workloads.station_iq on the other channels); channels in `loud` get the full level."""
    raster = raster or B
    centres = workloads.channel_grid(C, raster)
    kinds = kinds or ["AM"] * C
    tuner, ref = rc.Tuner(), oracle.Tuner()
    for f, k in zip(centres, kinds):
        tuner.add_channel(f, B, getattr(rc, k)(B, A))
        ref.add_channel(f, B, getattr(oracle, k)(B, A) if k != "AM" else None)
    tuner.request_bandwidth(float(N))
    ref.request_bandwidth(float(N))
    assert tuner.input_frequency == ref.input_frequency

    def band(buf):
        st = [am_model.station(i, B, seed=seed + 100 * buf, level=1.0 if i in loud else None) if k == "AM" else
              0.3 * workloads.station_iq(i + buf, B, deviation=0.2 * B, stereo=False) for i, k in enumerate(kinds)]
        return am_model.wideband(N, ref.input_frequency, centres, B, st, seed=seed + buf)
    return tuner, ref, band


def _check_channels(oracle, ref, got, idx, what=""):
    errs = {i: rel_err(got[i], am_model.expect_channel(oracle, ref, i, got.shape[1])) for i in idx}
    worst = max(errs, key=errs.get)
    print(what, "worst channel", worst, "rel err %.3g" % errs[worst])
    bad = {i: e for i, e in errs.items() if not e <= TOL}
    assert not bad, (what, bad)


def test_tuner_every_call_form(rc, oracle):
    """64 channels of 25 kHz: run_all, run_each and the per-channel loop AM.run(tuner.run(i)); the complex hand-over
    (phase_link=False: envelope kernel instead of the envelope link) and the unfused chain; two buffers."""
    N, B, A, C = 2_000_000, 25000, 8000, 64
    tuner, ref, band = _am_band(rc, oracle, C, B, A, N, seed=21)
    variants = [rc.Tuner() for _ in range(2)]
    for v in variants:
        for ch in tuner.channels():
            v.add_channel(ch.center_frequency, B, rc.AM(B, A))
        v.request_bandwidth(float(N))
    variants[0].set_kernel_options(phase_link=False)
    variants[1].set_kernel_options(fused_tiles=False)
    for buf in range(2):
        x = band(buf)
        ref.load(x)
        tuner.load(x)
        with _Profile() as ran:
            got = tuner.run_all()
        assert got.shape == (C, A, 1)
        # the envelope link: the tuner's last pass stored |x|, no envelope kernel ran
        assert ran["envelope"] == 0 and ran["am_tail"] >= 1 and ran["discriminator"] == 0, ran
        _check_channels(oracle, ref, got, range(C), "run_all")
        each = tuner.run_each()
        assert len(each) == C and all(e.shape == (A, 1) for e in each)
        for i in range(C):
            assert rel_err(each[i], got[i]) <= TOL, i
        for i in range(0, C, 5):
            loop = tuner.channels()[i].demodulator.run(tuner.run(i))
            assert rel_err(loop, got[i]) <= TOL, i
        for k, v in enumerate(variants):
            v.load(x)
            with _Profile() as ran:
                alt = v.run_all()
            if k == 0:
                assert ran["envelope"] >= 1, ran
            _check_channels(oracle, ref, alt, range(C), ("variant", k))


def test_mixed_run_each(rc, oracle):
    """MFM and FM channels next to AM ones of the same bandwidth: each group gets its own class's audio."""
    N, B, A, C = 1_000_000, 25000, 8000, 12
    kinds = ["AM"] * 3 + ["MFM"] * 3 + ["AM"] * 2 + ["FM"] * 2 + ["AM"] * 2
    tuner, ref, band = _am_band(rc, oracle, C, B, A, N, seed=5, kinds=kinds)
    x = band(0)
    tuner.load(x)
    ref.load(x)
    got = tuner.run_each()
    for i, k in enumerate(kinds):
        if k == "AM":
            want = am_model.expect_channel(oracle, ref, i, A)
        else:
            want = ref.channels()[i].demodulator.run(ref.run_pruned(i))
        assert got[i].shape == want.shape, (i, k)
        assert rel_err(got[i], want) <= TOL, (i, k)


# ---- the two FM paths AM must never take ---------------------------------------------------------------------------

def test_lds_chain_geometry_runs_am(rc, oracle):
    """12 500 -> 8000 is in lds_chain.hip's table: FM / MFM channels of that geometry run the LDS-resident chain,
    which computes the FM discriminator.  AM channels must take the multi-pass AM chain."""
    N, B, A, C = 1_000_000, 12500, 8000, 33
    tuner, ref, band = _am_band(rc, oracle, C, B, A, N, seed=9, raster=12500)
    x = band(0)
    tuner.load(x)
    ref.load(x)
    with _Profile() as ran:
        got = tuner.run_all()
    assert ran["lds_chain"] == 0 and ran["am_tail"] >= 1, ran
    _check_channels(oracle, ref, got, range(C), "lds geometry")


def test_two_pass_band_never_hands_am_phases(rc, oracle):
    """25 000 = 200 x 125 is a two-pass band whose rows of 200 samples would be handed over in padded phase rows to
    FM: AM's run_all must match the AM expectation (phases would give garbage) and must equal the complex hand-over."""
    N, B, A, C = 1_000_000, 25000, 8000, 9
    tuner, ref, band = _am_band(rc, oracle, C, B, A, N, seed=13)
    x = band(0)
    tuner.load(x)
    ref.load(x)
    linked = tuner.run_all()
    _check_channels(oracle, ref, linked, range(C), "two-pass")
    tuner.set_kernel_options(phase_link=False)
    plain = tuner.run_all()
    assert rel_err(linked, plain) <= 0.05 * TOL


# ---- full-size airband -----------------------------------------------------------------------------------------------

def test_airband_760_channels(rc, oracle):
    """VHF airband: 760 channels of 25 kHz (19 MHz) in a 20 MSPS buffer, run_all over two buffers; both ends and a
    seeded draw of 14 more are checked against the expectation.  The Tuner's wideband Hann window passes the two end
    channels at 0.7 % of their level, so they carry the full level: float32 rounding of the wideband FFT is relative
    to the whole band."""
    N, B, A, C = 20_000_000, 25000, 8000, 760
    tuner, ref, band = _am_band(rc, oracle, C, B, A, N, seed=31, loud=(0, C - 1))
    rng = np.random.default_rng(760)
    idx = [0, C - 1] + sorted(int(i) for i in rng.choice(np.arange(1, C - 1), 14, replace=False))
    print("checked channels:", idx)
    for buf in range(2):
        x = band(buf)
        tuner.load(x)
        got = tuner.run_all()
        assert got.shape == (C, A, 1) and not np.isnan(got).any()
        ref.load(x)
        _check_channels(oracle, ref, got, idx, ("airband", buf))
        del x


# ---- graph replay and Lanes ----------------------------------------------------------------------------------------

def test_graph_replay_is_bit_identical():
    import torch
    from radiocore._internal import hip
    lib = hip.lib()
    B, A = 25000, 8000
    handles = []
    for graph in (0, 1):
        h = ctypes.c_void_p()
        hip.check(lib.rcfm_demod_create(hip.RCFM_AM, 1, B, A, ctypes.c_double(75e-6), 0, ctypes.byref(h)))
        hip.check(lib.rcfm_demod_set_option(h, hip.RCFM_OPT_GRAPH, graph))
        handles.append(h)
    plain, graphed = handles
    bufs = [hip.to_device(am_model.station(i, B, seed=2).astype(np.complex64), torch.complex64) for i in range(3)]
    x = torch.empty_like(bufs[0])
    want, got = torch.empty(A, 1, device="cuda"), torch.empty(A, 1, device="cuda")
    s = hip.stream()
    for i in range(6):
        x.copy_(bufs[i % 3])
        hip.check(lib.rcfm_demod_run(plain, 0, 1, hip.ptr(x), hip.ptr(want), s))
        hip.check(lib.rcfm_demod_run(graphed, 0, 1, hip.ptr(x), hip.ptr(got), s))
        torch.cuda.synchronize()
        assert torch.equal(want, got), i
        assert float(want.abs().max()) > 1e-2
    v = ctypes.c_int()
    hip.check(lib.rcfm_demod_get_option(graphed, hip.RCFM_OPT_GRAPH, ctypes.byref(v)))
    assert v.value == 2, "the AM chain was not captured"
    for h in handles:
        hip.check(lib.rcfm_demod_destroy(h))


def test_lanes_equal_run_all(rc, oracle):
    from radiocore.tools import Lanes
    N, B, A, C = 1_000_000, 25000, 8000, 24
    tuner, ref, band = _am_band(rc, oracle, C, B, A, N, seed=40)
    bufs = [band(b) for b in range(4)]
    want = []
    for x in bufs:
        tuner.load(x)
        want.append(tuner.run_all())
    lanes_tuner, _, _ = _am_band(rc, oracle, C, B, A, N, seed=40)
    lanes = Lanes(lanes_tuner, depth=2)
    tickets = [lanes.submit(x) for x in bufs]
    got = [lanes.result(t) for t in tickets]
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (i, np.abs(g - w).max())
