"""GPU: weak AM / SSB channels paired with strong ones (tests/nearfar_model.py).

On the FFT-engine routes AM and SSB carry two channels in one complex transform; which two follows from channel order,
`first`, `chunk` and Tuner.shard -- nothing a user sees as signal content.  The reference demodulates every channel by
itself, so a channel's audio must not depend on what sits in the next row.  Every other AM / SSB test keeps the members
of a pair within 26 dB of each other; here the partner is 0, 42, 60 and 78 dB stronger (exact powers of two), on

    demodulator level   AM / USB / LSB (B, A, batch=5) on rows handed over directly: the decimating tile, the engine with
                        the separate resample, both engine routes of SSB, and the two rocFFT routes as unpaired controls
    with the AGC        the carried state keeps its absolute units: a weak row's is 2^-13 of the level-1 row's
    pipeline level      Tuner -> run_all over five adjacent channels, AM with the envelope link and without, USB straight
                        from the spectrum and from channel samples, against the float64 audio of the DEVICE's own
                        spectrum (read back after load), so the wideband float32 FFT's rounding -- which the reference
                        shares -- is taken out of the comparison; it is printed next to it

Bounds: TOL against the float64 expectation, ROUNDING (0.05 TOL, as tests/test_hip_signal_edges.py) between two HIP
evaluations of one result; the AGC chains at TOL for audio and state as tests/test_hip_agc.py checks its chains.
tests/test_nearfar_model.py shows that the reference alone stays within 0.1 TOL on every input used here and that a
float32 pair route without per-row scaling loses the weak rows at 78 dB.

Measured on an MI355X before the per-row scaling of csrc/pair_scale.hip, weak rows 1 and 2 (the model: 1.5e-4 / 6.5e-5 at
60 dB, 1.3e-3 / 6.8e-4 at 78 dB for AM): AM decimating tile 2.3e-4 / 1.4e-4 and 1.9e-3 / 1.2e-3, AM separate resample
1.9e-4 / 1.2e-4 and 1.4e-3 / 9.7e-4, USB 1.9e-4 / 2.4e-4 and 1.4e-3 / 1.7e-3, LSB 2.2e-4 / 2.1e-4 and 1.9e-3 / 1.6e-3; the
rocFFT controls, the strong rows, the lone last row and every level up to 42 dB passed.  With it every row of every
route is at its k = 0 error (<= 1.3e-6) at every level.
"""

import ctypes
import functools

import numpy as np
import pytest

import agc_model
import nearfar_model as nf
import radiocore_oracle as oracle
import signal_edges as se
from conftest import TOL, have_gpu, rel_err
from test_hip_am import _Profile

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ROUNDING = 0.05 * TOL


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


# ---- demodulator level -------------------------------------------------------------------------------------------------

# name: (kind, B, A, options switched off, engine plan for B?, stages that must have launched, stages that must not)
CASES = {
    "AM decimating tile": ("AM", 25000, 8000, (), True, ("envelope", "rfft_B", "ifft_A", "am_tail"), ("audio_spectrum",)),
    "AM separate resample": ("AM", 25000, 8000, ("RCFM_OPT_DECIM_TILE",), True,
                             ("envelope", "rfft_B", "audio_spectrum", "ifft_A", "am_tail"), ()),
    "AM rocFFT": ("AM", 22000, 8000, (), False, ("envelope", "rfft_B", "audio_spectrum", "ifft_A", "am_tail"), ()),
    "USB engine": ("USB", 12500, 8000, (), True, ("fft_B", "ifft_A", "ssb_tail"), ("audio_spectrum",)),
    "LSB engine": ("LSB", 12500, 8000, (), True, ("fft_B", "ifft_A", "ssb_tail"), ("audio_spectrum",)),
    "USB rocFFT": ("USB", 3001, 1001, (), False, ("fft_B", "audio_spectrum", "ifft_A", "ssb_tail"), ()),
}
CONTROLS = ("AM rocFFT", "USB rocFFT")


@functools.lru_cache(maxsize=None)
def _unit(kind, B, A, seed=nf.SEED):
    rows = nf.unit_rows(kind, B, A, seed)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _truth(kind, B, A, seed=nf.SEED):
    """Expected audio of the level-1 rows, float64 [5, A, 1]: computed once, shared by every level and route."""
    out = np.stack([nf.expect64(kind, x, B, A) for x in _unit(kind, B, A, seed)])
    out.setflags(write=False)
    return out


def _demod(rc, name, batch=nf.BATCH, **kw):
    from radiocore._internal import hip
    kind, B, A, off = CASES[name][:4]
    d = getattr(rc, kind)(B, A, batch=batch, **kw)
    for o in off:
        hip.check(hip.lib().rcfm_demod_set_option(d._handle.value, getattr(hip, o), 0))
    return d


@functools.lru_cache(maxsize=None)
def _five(name, k):
    """(audio [5, A, 1], stage profile) of the five rows of pattern(k) through one batched call of the case."""
    import radiocore
    kind, B, A = CASES[name][:3]
    d = _demod(radiocore, name)
    with _Profile() as ran:
        got = d.run(nf.scaled(_unit(kind, B, A), k))
    assert got.shape == (nf.BATCH, A, 1) and got.dtype == np.float32
    got.setflags(write=False)
    return got, dict(ran)


def _check_route(name, ran):
    from radiocore._internal import hip
    kind, B, A, off, engine, want, never = CASES[name]
    plan = hip.FftPlan()
    assert (hip.lib().rcfm_fft_describe(B, 0, ctypes.byref(plan)) == 0) == engine, (name, "engine plan for B")
    for st in want:
        assert ran[st] >= 1, (name, st, ran)
    for st in never + ("discriminator", "deemphasis", "lds_chain", "pilot_stage", "tuner_ifft_B"):
        assert ran[st] == 0, (name, st, ran)


@pytest.mark.parametrize("k", nf.LEVELS_K)
@pytest.mark.parametrize("name", list(CASES))
def test_every_row_whatever_its_partner(rc, name, k):
    """Rows [1, 2^-k, 2^-k, 1, 2^-k]: the weak member in the imaginary slot of its pair, in the real slot, and alone."""
    kind, B, A = CASES[name][:3]
    got, ran = _five(name, k)
    errs = [rel_err(got[i], _truth(kind, B, A)[i]) for i in range(nf.BATCH)]
    print(name, "k = %d:" % k, " ".join("%.2e" % e for e in errs), {s: n for s, n in ran.items() if n})
    _check_route(name, ran)
    assert not np.isnan(got).any()
    bad = {i: e for i, e in enumerate(errs) if not e <= TOL}
    assert not bad, (name, k, bad)


@pytest.mark.parametrize("k", [k for k in nf.LEVELS_K if k])
@pytest.mark.parametrize("name", CONTROLS)
def test_unpaired_controls_do_not_see_the_level(rc, name, k):
    """rocFFT transforms row by row: a weak row's audio is its k = 0 audio, within two HIP evaluations of one result."""
    base, _ = _five(name, 0)
    got, _ = _five(name, k)
    errs = {i: rel_err(got[i], base[i]) for i in nf.WEAK}
    print(name, "k = %d against k = 0:" % k, errs)
    assert max(errs.values()) <= ROUNDING, (name, k, errs)


@pytest.mark.parametrize("name", ["AM decimating tile", "USB engine", "LSB engine"])
def test_chunk_of_one_cannot_pair(rc, name):
    """A batch of two (strong, 78 dB weaker) with chunk = 1: every launch holds one row, nothing shares a transform.  The
    five-row run must give the same two rows."""
    kind, B, A = CASES[name][:3]
    rows = nf.scaled(_unit(kind, B, A), 13)[:2]
    alone = _demod(rc, name, batch=2, chunk=1).run(rows)
    five, _ = _five(name, 13)
    errs = [rel_err(five[i], alone[i]) for i in range(2)]
    truth = [rel_err(alone[i], _truth(kind, B, A)[i]) for i in range(2)]
    print(name, "five rows against chunk = 1: %.2e %.2e; chunk = 1 against float64: %.2e %.2e" % (*errs, *truth))
    assert max(truth) <= TOL, (name, truth)
    assert max(errs) <= ROUNDING, (name, errs)


# ---- with the stateful AGC -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["AM decimating tile", "USB engine"])
def test_agc_state_keeps_its_absolute_units(rc, name):
    """Two consecutive buffers of pattern(13) through agc=AGC(...): audio and carried state per row against
    agc_model.follow of agc_model.chain_signal.  The follower is in the signal's own units, so a weak row's state is
    2^-13 of what the same row carries at level 1 -- a scaling applied for the shared transform must be undone before the
    AGC sees the signal."""
    kind, B, A = CASES[name][:3]
    k = nf.AGC_K
    units, vs_unit, settings = nf.agc_case(kind, B, A)
    p = nf.pattern(k)
    floor = settings[2]
    mode = agc_model.chain_mode(kind)
    d = _demod(rc, name, agc=rc.AGC(agc_model.CHAIN_DECAY, floor=floor))
    got = [d.run(nf.scaled(u, k)) for u in units]
    state = d.agc_state()
    assert state.shape == (nf.BATCH,)
    for i in range(nf.BATCH):
        want, s_want = agc_model.follow([vs_unit[buf][i] * p[i] for buf in range(2)], mode, settings)
        _, s_unit = agc_model.follow([vs_unit[buf][i] for buf in range(2)], mode, settings)
        assert abs(s_want - s_unit * p[i]) <= 1e-12 * s_unit * p[i]      # the model's state does not see the floor
        ea = [rel_err(got[buf][i][:, 0], want[buf]) for buf in range(2)]
        es = agc_model.state_error(state[i], s_unit * p[i])
        print(name, "row", i, "audio %.2e %.2e  state %.2e (state %.6g, level-1 state %.6g)" % (*ea, es, state[i], s_unit))
        assert max(ea) <= TOL, (name, i, ea)
        assert es <= TOL, (name, i, es)


# ---- pipeline level ----------------------------------------------------------------------------------------------------

PIPELINE = {"AM": (1_000_000, 25000, 8000), "USB": (1_000_000, 12500, 8000)}
PIPELINE_K = (0, 10, 13)


@functools.lru_cache(maxsize=None)
def _band(kind, k):
    """(x complex64 [N], rolls, float64 audio of the IDEAL band per channel): five adjacent channels on the raster of
    signal_edges.centres_of, station amplitudes 0.3 pattern(k), no noise."""
    N, B, A = PIPELINE[kind]
    ref = se.oracle_tuner(B, nf.BATCH, N)
    x = se.wideband_from(list(_unit(kind, B, A)), N, ref.input_frequency, se.centres_of(B, nf.BATCH), B,
                         gain=0.3 * nf.pattern(k), noise=0.0)
    x.setflags(write=False)
    rolls = [ref._roll(i)[0] for i in range(nf.BATCH)]
    X = np.fft.fft(x.astype(np.complex128))
    ideal = [nf.from_spectrum(oracle, X, N, r, B, A, kind) for r in rolls]
    return x, rolls, ideal, ref.input_frequency


def _device_spectrum(tuner, N):
    from radiocore._internal import hip
    lib = hip.lib()
    X, halo, nn = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
    hip.check(lib.rcfm_tuner_spectrum_layout(tuner._handle.value, ctypes.byref(halo), ctypes.byref(nn)))
    assert nn.value == N
    hip.check(lib.rcfm_tuner_spectrum(tuner._handle.value, ctypes.byref(X)))
    host = np.empty(N, np.complex64)
    hip.check(lib.rcfm_memcpy_d2h(host.ctypes.data_as(ctypes.c_void_p), X, host.nbytes, hip.stream()))
    hip.check(lib.rcfm_stream_sync(hip.stream()))
    return host.astype(np.complex128)


@pytest.mark.parametrize("k", PIPELINE_K)
@pytest.mark.parametrize("kind,option", [("AM", "phase_link"), ("USB", "ssb_direct")])
def test_tuner_channels_against_the_devices_own_spectrum(rc, kind, option, k):
    """run_all with the option on and off (AM: the Tuner's last pass stores the envelope / the envelope kernel; USB: audio
    straight from the spectrum / from channel samples).  The expectation is the float64 audio of the spectrum the device
    itself holds: what is checked is the Tuner's gather and the pair routes, not the wideband FFT."""
    N, B, A = PIPELINE[kind]
    x, rolls, ideal, f_in = _band(kind, k)
    want = None
    for on in (True, False):
        tuner = rc.Tuner()
        for f in se.centres_of(B, nf.BATCH):
            tuner.add_channel(f, B, getattr(rc, kind)(B, A))
        tuner.request_bandwidth(float(N))
        assert tuner.input_frequency == f_in
        tuner.set_kernel_options(**{option: on})
        tuner.load(np.array(x))          # a copy: the shared band stays read-only
        if want is None:
            X = _device_spectrum(tuner, N)
            want = [nf.from_spectrum(oracle, X, N, r, B, A, kind) for r in rolls]
        with _Profile() as ran:
            got = tuner.run_all()
        assert got.shape == (nf.BATCH, A, 1) and not np.isnan(got).any()
        if kind == "AM":
            assert (ran["envelope"] == 0) == on and ran["am_tail"] >= 1, ran
        else:
            assert (ran["fft_B"] == 0) == on and ran["ssb_tail"] >= 1, ran
        errs = [rel_err(got[i], want[i]) for i in range(nf.BATCH)]
        floor = [rel_err(got[i], ideal[i]) for i in range(nf.BATCH)]
        print(kind, option, on, "k = %d" % k, "against the device's spectrum:", " ".join("%.2e" % e for e in errs),
              "| against the ideal band (the float32 wideband FFT's floor, not asserted):", " ".join("%.2e" % e for e in floor))
        bad = {i: e for i, e in enumerate(errs) if not e <= TOL}
        assert not bad, (kind, option, on, k, bad)
