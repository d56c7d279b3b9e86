"""GPU: the SSB demodulators (include/rcfm.h RCFM_USB / RCFM_LSB) against their specification, built from the oracle's
pieces (tests/ssb_model.py): one-sided spectral mask, radiocore_oracle.Decimate, RMS normalisation, clip.

Both routes -- audio straight from the Tuner's loaded spectrum (rcfm_pipeline_run) and from channel samples (USB.run /
LSB.run, and the pipeline with RCFM_OPT_SSB_DIRECT off or a geometry the fast gather refuses), on the FFT engine and
through rocFFT -- with the stage profile as evidence of which one ran; batches, odd channel counts and chunks, mixed
run_each, shard, graph replay, Lanes.

Tolerance: max|delta| <= 1e-4 * max|expected| (BASELINE.json north star), float32 end to end; no sample is excluded
(clipped ones are compared like the rest).  The RMS division amplifies whatever rounding error sits in an empty
sideband, so every compared sideband carries a signal over a noise floor of at least 1e-2 of it; in these bands it also
stays within 20 dB of the strongest one in the buffer (ssb_model.station; tests/test_ssb.py checks the seeded bands for
it).  That spread is what these bands happen to have, not a limit of the demodulators: tests/test_hip_nearfar.py runs
channels 78 dB apart through the same routes.
"""

import ctypes

import numpy as np
import pytest

import am_model
import ssb_model
import workloads
from conftest import TOL, have_gpu, rel_err
from test_hip_am import _Profile

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

B_TRANSFORMS = ("tuner_ifft_B", "rfft_B", "fft_B", "audio_spectrum")   # what the spectrum-direct route never launches
FM_ONLY = ("discriminator", "deemphasis", "deemph_state", "dc_clip", "lds_chain", "pilot_stage", "envelope", "am_tail")


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def oracle():
    import radiocore_oracle
    return radiocore_oracle


def _cls(rc, lower):
    return rc.LSB if lower else rc.USB


# ---- USB.run / LSB.run: the route from channel samples ---------------------------------------------------------------

STANDALONE = [
    # (B, A, batch, stages that must have launched besides ssb_tail)
    (12500, 8000, 1, ("fft_B", "ifft_A")),
    (12500, 8000, 5, ("fft_B", "ifft_A")),
    (25000, 8000, 1, ("fft_B", "ifft_A")),
    (25000, 8000, 4, ("fft_B", "ifft_A")),
    (240000, 48000, 3, ("fft_B", "ifft_A")),
    (250000, 48000, 1, ("fft_B", "ifft_A")),
    (240000, 44100, 2, ("fft_B", "ifft_A")),
    (3001, 1001, 1, ("fft_B", "audio_spectrum", "ifft_A")),      # prime B, 7 11 13: rocFFT
    (3001, 1001, 3, ("fft_B", "audio_spectrum", "ifft_A")),
    (22000, 8000, 2, ("fft_B", "audio_spectrum", "ifft_A")),     # 2^4 5^3 11: rocFFT
    (8000, 8000, 3, ("fft_B", "ifft_A")),                        # A = B, even: the bin B/2 is dropped
    (7875, 7875, 1, ("fft_B", "ifft_A")),                        # A = B, odd
    (4000, 6000, 3, ("fft_B", "ifft_A")),                        # A > B: Decimate's up-sampling rule
    (3001, 4002, 1, ("fft_B", "audio_spectrum", "ifft_A")),      # ... through rocFFT
]


@pytest.mark.parametrize("lower", [False, True], ids=["USB", "LSB"])
@pytest.mark.parametrize("B,A,batch,want", STANDALONE)
def test_standalone(rc, oracle, B, A, batch, want, lower):
    xs = np.stack([ssb_model.station(i, B, seed=3) for i in range(batch)]).astype(np.complex64)
    d = _cls(rc, lower)(B, A, batch=batch)
    with _Profile() as ran:
        got = d.run(xs[0] if batch == 1 else xs)
    got = got[None] if batch == 1 else got
    assert got.shape == (batch, A, 1) and got.dtype == np.float32
    errs = [rel_err(got[i], ssb_model.expect(oracle, xs[i], B, A, lower)) for i in range(batch)]
    print(B, A, batch, "LSB" if lower else "USB", "worst rel err %.3g" % max(errs), {k: v for k, v in ran.items() if v})
    assert max(errs) <= TOL, errs
    assert ran["ssb_tail"] == 1, ran
    for st in want:
        assert ran[st] >= 1, (st, ran)
    for st in FM_ONLY + ("rfft_B", "tuner_ifft_B") + (() if "audio_spectrum" in want else ("audio_spectrum",)):
        assert ran[st] == 0, (st, ran)


def test_each_class_hears_its_own_sideband(rc):
    B, A = 12500, 8000
    up = [(310.0, 1.0, 0.3), (1440.0, 0.6, 1.1)]
    lo = [(250.0, 0.8, 2.0), (2395.0, 0.7, 0.2)]
    x = ssb_model.ssb_iq(B, up, lo, level=0.05).astype(np.complex64)
    for lower, mine, other in ((False, up, lo), (True, lo, up)):
        audio = _cls(rc, lower)(B, A).run(x)
        spec = np.abs(np.fft.rfft(audio[:, 0].astype(np.float64))) / (A / 2)
        assert all(spec[int(f)] > 0.1 for f, _, _ in mine), (lower, spec[[int(f) for f, _, _ in mine]])
        assert all(spec[int(f)] < 1e-4 for f, _, _ in other), (lower, spec[[int(f) for f, _, _ in other]])
        assert abs(np.sqrt(np.mean(audio.astype(np.float64) ** 2)) - ssb_model.LEVEL) < 1e-5


@pytest.mark.parametrize("B,A", [(12500, 8000), (3001, 1001), (4000, 6000)])
def test_silent_channel_gives_zeros(rc, B, A):
    for cls in (rc.USB, rc.LSB):
        got = cls(B, A, batch=3).run(np.zeros((3, B), np.complex64))
        assert not np.isnan(got).any() and np.all(got == 0)


# ---- the Tuner -----------------------------------------------------------------------------------------------------

def _ssb_band(rc, oracle, kinds, B, A, N, seed, level=None):
    """A tuner and the oracle's over len(kinds) channels and a seeded band: two-sideband stations on the USB / LSB
    channels, AM stations (am_model) and FM stations (workloads.station_iq) on the others."""
    C = len(kinds)
    centres = workloads.channel_grid(C, B)
    tuner, ref = rc.Tuner(), oracle.Tuner()
    for f, k in zip(centres, kinds):
        tuner.add_channel(f, B, getattr(rc, k)(B, A))
        ref.add_channel(f, B, getattr(oracle, k)(B, A) if k in ("FM", "MFM") else None)
    tuner.request_bandwidth(float(N))
    ref.request_bandwidth(float(N))
    assert tuner.input_frequency == ref.input_frequency

    def band(buf):
        st = []
        for i, k in enumerate(kinds):
            if k in ("USB", "LSB"):
                st.append(ssb_model.station(i, B, seed=seed + 100 * buf, level=level))
            elif k == "AM":
                st.append(am_model.station(i, B, seed=seed + 100 * buf, level=0.5))
            else:
                st.append(0.5 * workloads.station_iq(i + buf, B, deviation=0.2 * B, stereo=False))
        return ssb_model.wideband(N, ref.input_frequency, centres, B, st, seed=seed + buf)
    return tuner, ref, band


def _expected(oracle, ref, i, kind, A):
    if kind in ("USB", "LSB"):
        return ssb_model.expect_channel(oracle, ref, i, A, kind == "LSB")
    if kind == "AM":
        return am_model.expect_channel(oracle, ref, i, A)
    return ref.channels()[i].demodulator.run(ref.run_pruned(i))


def _check(oracle, ref, got, kinds, idx, what="", first=0):
    """got[j] is channel first + j."""
    A = got[0].shape[0]
    errs = {i: rel_err(got[i - first], _expected(oracle, ref, i, kinds[i], A)) for i in idx}
    worst = max(errs, key=errs.get)
    print(what, "worst channel", worst, kinds[worst], "rel err %.3g" % errs[worst])
    bad = {i: e for i, e in errs.items() if not e <= TOL}
    assert not bad, (what, bad)
    return errs[worst]


@pytest.mark.parametrize("kind", ["USB", "LSB"])
@pytest.mark.parametrize("B,C,chunk", [(12500, 64, 0), (12500, 63, 0), (12500, 63, 20), (25000, 37, 7)])
def test_tuner_both_routes(rc, oracle, kind, B, C, chunk):
    """run_all through the spectrum-direct route and, with it switched off, through channel samples: the stage profile
    shows which one ran, both give the model's audio, and they agree with each other.  Odd channel counts and chunks
    leave an unpaired last channel in a launch."""
    N, A = 2_000_000, 8000
    kinds = [kind] * C
    tuner, ref, band = _ssb_band(rc, oracle, kinds, B, A, N, seed=21)
    general = rc.Tuner()
    for ch in tuner.channels():
        general.add_channel(ch.center_frequency, B, getattr(rc, kind)(B, A))
    general.request_bandwidth(float(N))
    general.set_kernel_options(ssb_direct=False)
    for buf in range(2):
        x = band(buf)
        ref.load(x)
        tuner.load(x)
        general.load(x)
        with _Profile() as ran:
            direct = tuner.run_all(chunk=chunk)
        launches = -(-C // chunk) if chunk else 1
        assert ran["ifft_A"] == launches and ran["ssb_tail"] == launches, ran
        for st in B_TRANSFORMS + FM_ONLY:
            assert ran[st] == 0, (st, ran)
        with _Profile() as ran:
            samples = general.run_all(chunk=chunk)
        for st in ("tuner_ifft_B", "fft_B", "ifft_A", "ssb_tail"):
            assert ran[st] == launches, (st, ran)
        for st in FM_ONLY + ("rfft_B", "audio_spectrum"):
            assert ran[st] == 0, (st, ran)
        assert direct.shape == samples.shape == (C, A, 1) and not np.isnan(direct).any()
        _check(oracle, ref, direct, kinds, range(C), (kind, "direct", buf))
        _check(oracle, ref, samples, kinds, range(C), (kind, "from samples", buf))
        between = max(rel_err(direct[i], samples[i]) for i in range(C))
        print("direct vs from samples: %.3g" % between)
        assert between <= TOL
        assert np.array_equal(direct, tuner.run_all(chunk=chunk))        # fixed summation order: bit-identical reruns
        assert np.array_equal(samples, general.run_all(chunk=chunk))


def test_wide_channels_fall_back_to_samples(rc, oracle):
    """A channel of an eighth of the band is outside the fast gather's window series: rcfm_pipeline_run takes the route
    from channel samples whatever the switch says."""
    N, B, A, C = 200_000, 25000, 8000, 5
    kinds = ["USB", "USB", "USB", "USB", "USB"]
    tuner, ref, band = _ssb_band(rc, oracle, kinds, B, A, N, seed=5)
    x = band(0)
    ref.load(x)
    tuner.load(x)
    with _Profile() as ran:
        got = tuner.run_all()
    assert ran["tuner_ifft_B"] == 1 and ran["fft_B"] == 1 and ran["ifft_A"] == 1 and ran["ssb_tail"] == 1, ran
    _check(oracle, ref, got, kinds, range(1, C - 1), "wide")   # the end channels sit under the Tuner's Hann skirt


def test_rocfft_geometry_under_the_pipeline(rc, oracle):
    """3001 -> 1001 has no engine plan on either side: tuner and demodulator both run rocFFT."""
    N, B, A, C = 90_000, 3001, 1001, 9
    kinds = ["LSB"] * C
    tuner, ref, band = _ssb_band(rc, oracle, kinds, B, A, N, seed=6)
    x = band(0)
    ref.load(x)
    tuner.load(x)
    with _Profile() as ran:
        got = tuner.run_all()
    assert ran["audio_spectrum"] == 1 and ran["ssb_tail"] == 1, ran
    _check(oracle, ref, got, kinds, range(C), "rocFFT pipeline")


def test_run_each_next_to_am_and_fm(rc, oracle):
    """USB and LSB groups between AM and FM neighbours: one batched sequence per group, each by its own chain."""
    N, B, A = 2_000_000, 25000, 8000
    kinds = ["USB"] * 3 + ["AM"] * 2 + ["LSB"] * 5 + ["FM"] * 2 + ["USB"] + ["LSB"] * 2 + ["AM"] + ["USB"] * 4
    tuner, ref, band = _ssb_band(rc, oracle, kinds, B, A, N, seed=8, level=1.0)
    for buf in range(2):
        x = band(buf)
        tuner.load(x)
        ref.load(x)
        with _Profile() as ran:
            got = tuner.run_each()
        assert ran["ssb_tail"] == 5 and ran["am_tail"] == 2, ran
        assert all(g.shape == (A, 1) for g in got)
        _check(oracle, ref, got, kinds, range(len(kinds)), ("run_each", buf))


def test_after_shard(rc, oracle):
    """shard(first, count): only that range runs, straight from the spectrum rows the sharded load kept."""
    N, B, A, C = 2_000_000, 12500, 8000, 64
    kinds = ["USB" if (i // 4) % 2 == 0 else "LSB" for i in range(C)]
    uniform = ["LSB"] * C
    for ks, call in ((uniform, "run_all"), (kinds, "run_each")):
        tuner, ref, band = _ssb_band(rc, oracle, ks, B, A, N, seed=12)
        x = band(0)
        ref.load(x)
        tuner.load(x)
        whole = getattr(tuner, call)()
        tuner.shard(21, 23)
        tuner.load(x)
        with _Profile() as ran:
            part = getattr(tuner, call)()
        assert len(part) == 23 and ran["tuner_ifft_B"] == 0 and ran["ssb_tail"] >= 1, ran
        _check(oracle, ref, part, ks, range(21, 44), ("shard", call), first=21)
        assert max(rel_err(part[j], whole[21 + j]) for j in range(23)) <= TOL


def test_hf_band_760_channels(rc, oracle):
    """760 channels of 25 kHz in a 20 MSPS buffer (the AM airband geometry), alternating sidebands in run_each and one
    sideband in run_all, two buffers; both ends and a seeded draw of 14 more are checked."""
    N, B, A, C = 20_000_000, 25000, 8000, 760
    rng = np.random.default_rng(761)
    idx = [0, C - 1] + sorted(int(i) for i in rng.choice(np.arange(1, C - 1), 14, replace=False))
    print("checked channels:", idx)
    worst = 0.0
    for kinds, call in ((["USB"] * C, "run_all"), (["LSB"] * C, "run_all"),
                        (["USB" if i % 2 == 0 else "LSB" for i in range(C)], "run_each")):
        tuner, ref, band = _ssb_band(rc, oracle, kinds, B, A, N, seed=31)
        for buf in range(2 if call == "run_all" and kinds[0] == "USB" else 1):
            x = band(buf)
            tuner.load(x)
            with _Profile() as ran:
                got = getattr(tuner, call)()
            for st in B_TRANSFORMS:
                assert ran[st] == 0, (st, ran)
            assert len(got) == C and not np.isnan(np.asarray(got)).any()
            ref.load(x)
            worst = max(worst, _check(oracle, ref, got, kinds, idx, (call, kinds[1], buf)))
            del x
    print("worst of the 760-channel band: %.3g" % worst)


# ---- graph replay and Lanes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["RCFM_USB", "RCFM_LSB"])
def test_graph_replay_is_bit_identical(kind):
    import torch
    from radiocore._internal import hip
    lib = hip.lib()
    B, A = 25000, 8000
    handles = []
    for graph in (0, 1):
        h = ctypes.c_void_p()
        hip.check(lib.rcfm_demod_create(getattr(hip, kind), 1, B, A, ctypes.c_double(75e-6), 0, ctypes.byref(h)))
        hip.check(lib.rcfm_demod_set_option(h, hip.RCFM_OPT_GRAPH, graph))
        handles.append(h)
    plain, graphed = handles
    bufs = [hip.to_device(ssb_model.station(i, B, seed=2).astype(np.complex64), torch.complex64) for i in range(3)]
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
    assert v.value == 2, "the SSB chain was not captured"
    for h in handles:
        hip.check(lib.rcfm_demod_destroy(h))


def test_lanes_equal_run_all(rc, oracle):
    from radiocore.tools import Lanes
    N, B, A, C = 1_000_000, 12500, 8000, 25
    kinds = ["USB"] * C
    tuner, ref, band = _ssb_band(rc, oracle, kinds, B, A, N, seed=40)
    bufs = [band(b) for b in range(4)]
    want = []
    for x in bufs:
        tuner.load(x)
        want.append(tuner.run_all())
    lanes_tuner, _, _ = _ssb_band(rc, oracle, kinds, B, A, N, seed=40)
    lanes = Lanes(lanes_tuner, depth=2)
    tickets = [lanes.submit(x) for x in bufs]
    got = [lanes.result(t) for t in tickets]
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (i, np.abs(g - w).max())


def test_all_zero_buffer_gives_exact_zeros(rc):
    N, B, A, C = 1_000_000, 12500, 8000, 11
    for kind, direct in (("USB", True), ("LSB", True), ("USB", False)):
        tuner = rc.Tuner()
        for f in workloads.channel_grid(C, B):
            tuner.add_channel(f, B, getattr(rc, kind)(B, A))
        tuner.request_bandwidth(float(N))
        tuner.set_kernel_options(ssb_direct=direct)
        tuner.load(np.zeros(N, np.complex64))
        got = tuner.run_all()
        assert got.shape == (C, A, 1) and not np.isnan(got).any() and np.all(got == 0)


# ---- the example -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plan", ["split", "usb", "lsb"])
def test_hf_ssb_example(plan):
    """examples/hf_ssb.py: a 150-channel HF band at 2 MSPS, one sideband per half of the band (run_each) or one
    everywhere (run_all), through the wire framing; every sampled station's tone sits at RCFM_SSB_LEVEL sqrt(2)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("hf_ssb", os.path.join(root, "examples", "hf_ssb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sent = []
    msgs, worst = mod.run(channels=150, seconds=2, plan=plan, publish=sent.append)
    assert len(msgs) == len(sent) == 300
    assert all(p.shape == (8000, 1) and p.dtype == np.float32 for _, p in msgs)
    assert sorted({f for f, _ in msgs})[0] == 10_000_000 - 75 * 12500 + 6250
    rms = [float(np.sqrt(np.mean(p.astype(np.float64) ** 2))) for _, p in msgs]
    assert max(abs(r - ssb_model.LEVEL) for r in rms) < 1e-5
    print(plan, "tone amplitude within %.2e of %.4f" % (worst, ssb_model.LEVEL * np.sqrt(2)))
    assert worst < 2e-3
