"""CPU: the SSB demodulators' surface (include/rcfm.h RCFM_USB / RCFM_LSB, radiocore.USB / LSB, Tuner bookkeeping) --
librcfm.so loaded, no device used -- and the numpy model the GPU tests compare against (tests/ssb_model.py)."""

import ctypes
import os
import re

import numpy as np
import pytest

import radiocore_oracle as oracle
import ssb_model
from test_am import _CountingLib, _FakeTensor, _FakeTorch  # noqa: F401  (the same stand-ins as the AM surface tests)

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "rcfm.h")
TOOLS_HEADER = os.path.join(os.path.dirname(HERE), "include", "rcfm_tools.h")


@pytest.fixture(scope="module")
def hip():
    from radiocore._internal import hip
    hip.lib()
    return hip


def test_kinds_and_level_in_the_header_and_the_binding(hip):
    text = open(HEADER).read()
    for name, value in (("RCFM_USB", 5), ("RCFM_LSB", 6)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
        assert m is not None and int(m.group(1)) == value
        assert getattr(hip, name) == value
    assert re.search(r"=\s*4\b", text.split("typedef enum rcfm_demod_kind")[1].split("}")[0]) is None   # 4 stays free
    m = re.search(r"#define\s+RCFM_SSB_LEVEL\s+([0-9.]+)f", text)
    assert m is not None and float(m.group(1)) == hip.RCFM_SSB_LEVEL == ssb_model.LEVEL == 0.25
    m = re.search(r"\bRCFM_OPT_SSB_DIRECT\s*=\s*(\d+)", open(TOOLS_HEADER).read())
    assert m is not None and int(m.group(1)) == hip.RCFM_OPT_SSB_DIRECT == 11
    assert hip.lib().rcfm_version() == 102


def test_create_accepts_both_kinds_as_far_as_the_size_checks(hip):
    lib = hip.lib()
    h = ctypes.c_void_p()
    for kind in (5, 6):
        assert lib.rcfm_demod_create(kind, 1, 100, 0, ctypes.c_double(75e-6), 0, ctypes.byref(h)) == -4
        assert b"bad demodulator size" in lib.rcfm_last_error()
    for kind in (4, 7):
        assert lib.rcfm_demod_create(kind, 1, 100, 50, ctypes.c_double(75e-6), 0, ctypes.byref(h)) == -4
        assert b"kind" in lib.rcfm_last_error()


@pytest.fixture()
def no_device(monkeypatch):
    """The package's Python layer without a device: torch and the ABI replaced by stand-ins (no compute call)."""
    from radiocore._internal import hip
    lib = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: lib)
    monkeypatch.setattr(hip, "torch", lambda: _FakeTorch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _FakeTensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _FakeTensor(getattr(x, "shape", (len(x),))))
    monkeypatch.setattr(hip, "to_host", lambda x: x)
    return lib


def test_class_surface(no_device):
    import radiocore
    from radiocore import LSB, USB
    from radiocore.analog import LSB as LSB2, USB as USB2
    from radiocore._internal import hip
    assert USB is USB2 is radiocore.analog.ssb.USB and LSB is LSB2 is radiocore.analog.ssb.LSB
    assert (USB._KIND, LSB._KIND) == (hip.RCFM_USB, hip.RCFM_LSB)
    for cls in (USB, LSB):
        assert cls(12500, 8000).channels == 1
        assert cls(12500, 8000, deemphasis=50e-6, batch=4, chunk=2).channels == 1
        for bad in [dict(input_size=1, output_size=8000), dict(input_size=12500, output_size=0),
                    dict(input_size=12500, output_size=8000, batch=0)]:
            with pytest.raises(ValueError):
                cls(**bad)


def _tuner(kinds, B=12500, A=8000):
    import radiocore as rc
    t = rc.Tuner()
    for i, k in enumerate(kinds):
        t.add_channel(7.0e6 + float(B) * i, B, getattr(rc, k)(B, A))
    t.request_bandwidth(2_000_000.0)
    return t


def test_tuner_geometry_and_plan(no_device):
    import radiocore as rc
    from radiocore._internal import hip
    from radiocore.tools.tuner import Tuner
    assert Tuner._geometry(rc.USB(12500, 8000)) == (5, 12500, 8000, 75e-6)
    assert Tuner._geometry(rc.LSB(12500, 8000)) == (6, 12500, 8000, 75e-6)
    t = _tuner(["USB"] * 3 + ["LSB"] * 2 + ["USB"])
    groups, first, count = t._launch_plan()
    assert (first, count) == (0, 6)
    assert [g[:3] for g in groups] == [(0, 3, hip.RCFM_USB), (3, 2, hip.RCFM_LSB), (5, 1, hip.RCFM_USB)]
    assert t._plan_uniform() is None
    assert _tuner(["LSB"] * 4)._plan_uniform() == (hip.RCFM_LSB, 12500, 8000, 75e-6)


def test_run_all_is_one_pipeline_call_and_refuses_mixed_sidebands(no_device):
    lib = no_device
    t = _tuner(["USB"] * 5)
    t.load(np.zeros(2_000_000, np.complex64))
    t.run_all()
    assert [args[0] for n, args in lib.calls if n == "rcfm_demod_create"] == [5]
    assert lib.count("rcfm_pipeline_run") == 1
    assert lib.count("rcfm_demod_bind_state") == 0
    t = _tuner(["USB", "LSB"])
    t.load(np.zeros(2_000_000, np.complex64))
    with pytest.raises(ValueError, match="one demodulator class and geometry"):
        t.run_all()


def test_mixed_run_each_needs_no_state_binding_or_fence(no_device):
    """run_each over USB | MFM | LSB | AM | FM | USB: only the MFM group binds state and takes the Lanes fence."""
    from radiocore._internal import hip
    lib = no_device
    t = _tuner(["USB"] * 2 + ["MFM"] * 2 + ["LSB"] * 2 + ["AM", "FM", "USB"])
    t.load(np.zeros(2_000_000, np.complex64))
    out = t.run_each()
    assert len(out) == 9
    kinds = [args[0] for n, args in lib.calls if n == "rcfm_demod_create"]
    assert sorted(kinds) == sorted([hip.RCFM_USB, hip.RCFM_MFM, hip.RCFM_LSB, hip.RCFM_AM, hip.RCFM_FM])
    assert lib.count("rcfm_pipeline_run") == 6
    assert [c.demodulator._binding is None for c in t.channels()] == [True] * 2 + [False] * 2 + [True] * 5
    assert all(k[0] == hip.RCFM_MFM for k in t._state_owner)
    lib.calls.clear()
    t._arm_state_fence()
    fenced = [args for n, args in lib.calls if n == "rcfm_demod_set_option" and args[1] == hip.RCFM_OPT_STATE_FENCE]
    assert len(fenced) == 1
    lib.calls.clear()
    assert t.run_each() and lib.count("rcfm_demod_bind_state") == 0


def test_direct_switch_reaches_the_batched_handle(no_device):
    from radiocore._internal import hip
    lib = no_device
    t = _tuner(["USB"] * 3)
    t.set_kernel_options(ssb_direct=False)
    t.load(np.zeros(2_000_000, np.complex64))
    t.run_all()
    sets = [args[1:] for n, args in lib.calls if n == "rcfm_demod_set_option"]
    assert sets == [(hip.RCFM_OPT_SSB_DIRECT, 0)]


def test_run_each_error_names_the_classes(no_device):
    import radiocore as rc
    t = rc.Tuner()
    t.add_channel(7.0e6, 12500, rc.USB(12500, 8000))
    t.add_channel(7.0125e6, 12500, None)
    t.request_bandwidth(2_000_000.0)
    t.load(np.zeros(2_000_000, np.complex64))
    with pytest.raises(ValueError, match="USB or LSB"):
        t.run_each()


# ---- the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,B,A", [(200000, 12500, 8000), (200000, 25000, 8000), (90000, 3001, 1001), (90000, 3000, 1001),
                                   (90000, 3001, 1000), (90000, 3000, 3000), (90001, 3001, 3001)])
def test_direct_formula_equals_the_composed_model(N, B, A):
    """The audio spectrum picked straight out of the Tuner's loaded spectrum gives the v of the composed model
    (Tuner channel -> sideband mask -> Decimate) on every channel, both sidebands.  The model rounds the channel samples
    to complex64 on the way, the direct formula does not: 4e-6 of peak at most with in-band signals like these."""
    t = oracle.Tuner()
    C = N // B - 1
    for c in range(C):
        t.add_channel(7.0e6 + c * B, B, None)
    t.request_bandwidth(float(N))
    rng = np.random.default_rng(1)
    x = 0.3 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    tt = np.arange(N) / N
    off = t.channels()[2].center_frequency - t.input_frequency
    for f, a in ((700, 1.0), (1900, 0.5), (-1200, 0.8)):
        x = x + a * np.exp(2j * np.pi * (off + f) * tt)
    t.load(x.astype(np.complex64))
    worst = clipped = 0.0
    for lower in (False, True):
        for c in range(C):
            v = ssb_model.sideband(oracle, t.run_pruned(c), B, A, lower)
            d = ssb_model.direct(oracle, t._buffer, t._roll(c)[0], B, A, lower)
            worst = max(worst, float(np.max(np.abs(d - v)) / np.max(np.abs(v))))
            clipped = max(clipped, float(np.mean(np.abs(ssb_model.normalise(v)) >= 0.999)))
    assert worst <= 1e-5, worst
    assert clipped <= 0.02, clipped


def _line(audio, f):
    """Amplitude of the spectral line at f Hz of a one-second audio buffer."""
    a = np.asarray(audio)[:, 0]
    return float(np.abs(np.fft.rfft(a))[int(f)] / (len(a) / 2))


@pytest.mark.parametrize("B,A", [(12500, 8000), (3001, 1001), (8000, 8000), (4000, 6000)])
def test_each_class_hears_its_own_sideband(B, A):
    """Tones above the centre come out of USB at their own frequencies with the amplitudes Decimate's Hamming weight
    predicts after the RMS normalisation; LSB hears the tones below the centre instead, and none of the others."""
    up = [(310.0, 1.0, 0.3), (440.0, 0.6, 1.1)]
    lo = [(250.0, 0.8, 2.0), (395.0, 0.7, 0.2), (120.0, 0.5, 4.0)]
    x = ssb_model.ssb_iq(B, up, lo, level=3.0)
    W = oracle.shifted_window("hamm", B)
    for lower, mine, other in ((False, up, lo), (True, lo, up)):
        audio = ssb_model.expect(oracle, x, B, A, lower)
        amp = np.array([a * 0.5 * (W[int(f)] + W[B - int(f)]) for f, a, _ in mine])
        g = np.sqrt(np.sum(amp ** 2) / 2.0)
        assert np.max(np.abs(audio)) < 0.999
        for (f, _, _), want in zip(mine, ssb_model.LEVEL * amp / g):
            assert abs(_line(audio, f) - want) <= 2e-6 * want, (lower, f)
        for f, _, _ in other:
            assert _line(audio, f) <= 1e-6, (lower, f)
        assert abs(np.sqrt(np.mean(audio ** 2)) - ssb_model.LEVEL) <= 1e-6
        assert abs(np.mean(audio)) <= 1e-9


def test_audio_does_not_depend_on_the_station_level():
    B, A = 12500, 8000
    up, lo = ssb_model.station_tones(3)
    ref = ssb_model.expect(oracle, ssb_model.ssb_iq(B, up, lo, 1.0, 0.02, seed=5), B, A, False)
    for level in (1e-3, 40.0):
        got = ssb_model.expect(oracle, ssb_model.ssb_iq(B, up, lo, level, 0.02, seed=5), B, A, False)
        assert np.max(np.abs(got - ref)) <= 2e-6      # the complex64 rounding of the samples
    assert not np.any(ssb_model.expect(oracle, np.zeros(B, np.complex64), B, A, True))


def test_seeded_band_keeps_the_condition_on_the_inputs():
    """Every sideband of every station of a seeded band lies within 20 dB of the strongest signal, over a noise floor of
    at least 1e-2 of it (what the GPU comparisons assume, tests/test_hip_ssb.py)."""
    peak = []
    for i in range(64):
        up, lo = ssb_model.station_tones(i, seed=2)
        rng = np.random.default_rng(5000 + 2000 + i)
        level = 10.0 ** rng.uniform(-0.7, 0.0)
        for side in (up, lo):
            peak.append((level * min(a for _, a, _ in side), level * max(a for _, a, _ in side), 0.02 * level))
    strongest = max(p[1] for p in peak)
    assert all(p[0] >= 0.1 * strongest for p in peak)
    assert all(p[2] >= 1e-2 * p[1] for p in peak)
