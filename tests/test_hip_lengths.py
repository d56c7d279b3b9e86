"""GPU: FM / MFM / WBFM / AM at odd, equal and up-sampling channel lengths (tests/length_cases.py has the table, the
stations, the float64 truth and the bound; tests/test_length_cases.py pins them without a GPU).

Batched single calls -- rc.<kind>(B, A, batch=3).run(xs): three different stations, two consecutive buffers (the
de-emphasis state of MFM / WBFM is carried), one test per case:
    audio vs the float64 truth   <= length_cases.bound(case) = min(TOL, smallest mutant distance / 10)
    audio vs the oracle          <= TOL
The route is never assumed.  Per case the test collects the plan or refusal rcfm_fft_describe gives for B and A and the
stage profile of the second buffer: the rocFFT WBFM route shows hilbert_mask and stereo_mix, the engine route neither;
dc_clip runs on its own where the route left no DC bin (rocFFT) or the audio rows are no whole quads (A ch % 4 != 0);
one pilot_stage per chunk.  Which restatement of the resampling rule ran is read from the profile too and held to
length_cases.resample_site: the decimating tile (no audio_spectrum stage; for WBFM no ifft_A stage), a resampling
kernel (the audio_spectrum stage: FM / MFM / AM, and WBFM on rocFFT) or, for WBFM on the engine, the load of IFFT_A's
first pass -- run_wbfm_engine has no audio_spectrum stage at all, its ifft_A stage is the mark; where no decimating
tile can apply (A >= B, odd A, rocFFT) the tile must not have run.  The one rule behind the site is
length_cases.tile_of -- the tile's form and its two lengths (L, L2), which tests/test_length_cases.py holds to the routing
restated in tests/decim_cases.py; tests/test_hip_decim_lengths.py takes the tile to every other long length.  The pilot kernel form comes from B and from the
EFFECTIVE RCFM_OPT_PILOT_BLOCKED the handle reports: tile-blocked, k_pilot_stage_h40 owns whole rows and its branch "the
channel ends inside this thread's run" is never taken, so a case labelled "h40_ragged" must report 0.
test_every_cell_of_the_table_was_reached holds the collected (branch, route, pilot kernel) set against the table: a
planner change that silently moves a case shows up there.

Measured on an MI355X (the table of length_cases.py has every case): FM / MFM <= 8.8e-7 of peak against the truth on
either route, AM <= 1.6e-6 on the engine and <= 3.3e-6 on rocFFT, WBFM <= 3.5e-6 on the engine (62 500 -> 12 500; the
others <= 1.4e-6) and <= 1.1e-6 on rocFFT, against bounds of 2.5e-5 .. 1e-4.  Through the Tuner <= 2.0e-6 on the default
route and <= 8.1e-6 on the plain one (WBFM 62 500 -> 12 500: the discriminator on complex64 samples instead of phases).

Through the Tuner -- rc.Tuner against radiocore_oracle.Tuner, the band built by signal_edges.wideband_from from the same
stations: C = 3, chunk = 2 (a lone last pair member), two buffers, N = 10 int(1.25 B).  Each case runs on a second Tuner
with set_kernel_options(fused_tiles=False, phase_link=False) as well; both must lie within the bound of the truth and of
each other.  A third Tuner with phase_link=False alone shows whether the default took the phase (envelope) link:
rcfm_demod_get_option returns that switch as set, and WBFM's stage profile does not tell the two inputs of the pilot
kernel apart, so the evidence is demod.hip's phase_capable() restated from the plan (length_cases.phase_capable) plus
the audio -- it differs in rounding from the default's where the link was taken (62 500 -> 12 500: 1.4e-6 against
8.2e-7 from the truth) and is bit-identical where it was not (60 750, 50 625).  For the WBFM cases the effective
RCFM_OPT_PILOT_BLOCKED is asserted 0: that is what puts IN = float through the ragged-end branch at 62 500.
"""

import ctypes

import numpy as np
import pytest

import length_cases as lc
import signal_edges as se
import workloads
from conftest import TOL, have_gpu, rel_err
from test_hip_am import _Profile

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

IDS = ["%s-%d-%d" % c for c in lc.CASES]
_RESULTS = {}       # case -> (errors vs truth, vs oracle, stage launches of the last buffer, engine plans B and A?, blocked)


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


def _planned(n):
    from radiocore._internal import hip
    plan = hip.FftPlan()
    return hip.lib().rcfm_fft_describe(n, 0, ctypes.byref(plan)) == 0


def _run_case(rc, case):
    """The batched call of `case` over both buffers, once per session."""
    if case in _RESULTS:
        return _RESULTS[case]
    kind, B, A = case
    ch = lc.channels(kind)
    demod = getattr(rc, kind)(B, A, batch=lc.ROWS)
    refs = [lc.reference(kind, B, A) for _ in range(lc.ROWS)]
    want = lc.truths(kind, B, A)
    e_truth, e_ref, ran = [], [], {}
    for buf, x in enumerate(lc.signals(kind, B, A)):
        if buf == lc.BUFFERS - 1:
            with _Profile() as ran:
                got = demod.run(x.copy())        # (the cached signals are read-only: torch wants a writable array)
        else:
            got = demod.run(x.copy())
        got = np.asarray(got)
        assert got.shape == (lc.ROWS, A, ch) and got.dtype == np.float32, (got.shape, got.dtype)
        for r in range(lc.ROWS):
            e_truth.append(rel_err(got[r], want[buf][r]))
            e_ref.append(rel_err(got[r], refs[r].run(x[r])))
    # the EFFECTIVE tile-blocked hand-over of m and p (WBFM): with it k_pilot_stage_h40 owns whole rows and never takes
    # the branch "the channel ends inside this thread's run"
    blocked = _handle_option(demod._handle.value, "RCFM_OPT_PILOT_BLOCKED") if kind == "WBFM" else 0
    _RESULTS[case] = (e_truth, e_ref, {k: v for k, v in ran.items() if v}, (_planned(B), _planned(A)), blocked)
    return _RESULTS[case]


def _handle_option(handle, name):
    from radiocore._internal import hip
    v = ctypes.c_int(-1)
    hip.check(hip.lib().rcfm_demod_get_option(handle, getattr(hip, name), ctypes.byref(v)))
    return v.value


def _resample_site(kind, route, ran):
    """Which restatement of the resampling rule ran (length_cases.resample_site), from the stage profile."""
    if kind == "WBFM" and route == "engine":
        assert ran.get("audio_spectrum", 0) == 0, ran        # run_wbfm_engine has no such stage
        return "ifft_load" if ran.get("ifft_A", 0) else "decim_tile"
    assert ran.get("ifft_A", 0) >= 1, ran
    return "resample_kernel" if ran.get("audio_spectrum", 0) else "decim_tile"


def _route_of(case):
    """(branch, route, pilot kernel) from what the library reported and launched, with the stage profile checked."""
    kind, B, A = case
    _, _, ran, planned, blocked = _RESULTS[case]
    route = "engine" if all(planned) else "rocfft"
    if kind == "WBFM":
        assert ran.get("pilot_stage", 0) == 1, (case, ran)                      # one chunk
        rocfft_stages = [ran.get(k, 0) for k in ("hilbert_mask", "stereo_mix")]
        assert all(rocfft_stages) if route == "rocfft" else not any(rocfft_stages), (case, route, ran)
    else:
        assert ran.get("pilot_stage", 0) == 0 and ran.get("lds_chain", 0) == 0, (case, ran)
        assert ran.get("envelope" if kind == "AM" else "discriminator", 0) == 1, (case, ran)
    site = _resample_site(kind, route, ran)
    assert site == lc.resample_site(kind, B, A), (case, site, ran)
    if route == "rocfft" or A >= B or A % 2:
        assert site != "decim_tile", (case, ran)                                # no decimating tile can apply
    if kind in ("MFM", "WBFM"):
        # the de-emphasis takes its mean from the DC bin and clips in the same kernel, unless the route left no DC bin
        # (rocFFT) or the audio rows are no whole 16-byte quads: then the generic FIR and a dc_clip launch of its own
        assert (ran.get("dc_clip", 0) >= 1) == (route == "rocfft" or (A * lc.channels(kind)) % 4 != 0), (case, ran)
    if blocked:
        assert route == "engine" and B % 4 == 0, (case, blocked)
    return lc.branch(B, A), route, lc.pilot_kernel(kind, B, blocked)


@pytest.mark.parametrize("kind,B,A", list(lc.CASES), ids=IDS)
def test_batched_call(rc, kind, B, A):
    case = (kind, B, A)
    bound = lc.bound(kind, B, A)
    e_truth, e_ref, ran, planned, blocked = _run_case(rc, case)
    route = _route_of(case)
    print("%s %d -> %d: %s, %s %s, engine plans (B, A) %s, pilot blocked %d, vs truth %.2e (bound %.2e), vs oracle %.2e, stages %s"
          % (kind, B, A, route, lc.resample_site(kind, B, A), lc.tile_of(kind, B, A) or "", planned, blocked, max(e_truth),
             bound, max(e_ref), ran))
    assert route == lc.CASES[case], (case, route)
    assert max(e_truth) <= bound, (case, e_truth, bound)
    assert max(e_ref) <= TOL, (case, e_ref)


def test_every_cell_of_the_table_was_reached(rc):
    reached = set()
    for case in lc.CASES:
        _run_case(rc, case)
        reached.add((case[0],) + _route_of(case))
    for kind in ("FM", "MFM", "WBFM"):
        cells = {(r, b) for k, b, r, _ in reached if k == kind}
        assert cells == {(r, b) for r in ("engine", "rocfft") for b in lc.BRANCHES}, (kind, cells)
    assert {(r, b) for k, b, r, _ in reached if k == "AM"} >= {
        (r, b) for r in ("engine", "rocfft") for b in ("down_even", "same_even", "same_odd", "up_even", "up_odd")}
    pilots = {(r, p) for k, _, r, p in reached if k == "WBFM"}
    assert pilots >= {("engine", "h40_blocked"), ("engine", "h40_ragged"), ("engine", "generic_even"), ("engine", "generic_odd"),
                      ("rocfft", "h40_ragged"), ("rocfft", "generic_even"), ("rocfft", "generic_odd")}, pilots
    assert reached == {(k[0],) + v for k, v in lc.CASES.items()}


# ---- through the Tuner ------------------------------------------------------------------------------------------------------

def _option(tuner, option):
    """The value rcfm_demod_get_option reports on the tuner's one batched handle (the effective one where the library
    defines it so)."""
    from radiocore._internal import hip
    assert len(tuner._batched) == 1, list(tuner._batched)
    v = ctypes.c_int(-1)
    hip.check(hip.lib().rcfm_demod_get_option(next(iter(tuner._batched.values())).value, option, ctypes.byref(v)))
    return v.value


@pytest.mark.parametrize("kind,B,A", lc.TUNER_CASES, ids=["%s-%d-%d" % c for c in lc.TUNER_CASES])
def test_through_the_tuner(rc, kind, B, A):
    import radiocore_oracle as oracle
    from radiocore._internal import hip
    C, chunk = 3, 2
    raster = int(1.25 * B)
    N = 10 * raster
    ch = lc.channels(kind)
    bound = lc.bound(kind, B, A)
    centres = workloads.channel_grid(C, raster)
    tuners = [rc.Tuner(), rc.Tuner(), rc.Tuner()]
    tuners[1].set_kernel_options(fused_tiles=False, phase_link=False)
    tuners[2].set_kernel_options(phase_link=False)       # the default kernels behind a complex hand-over
    ref = oracle.Tuner()
    for f in centres:
        for t in tuners:
            t.add_channel(f, B, getattr(rc, kind)(B, A))
        ref.add_channel(f, B, None)
    for t in tuners + [ref]:
        t.request_bandwidth(float(N))
    assert tuners[0].input_frequency == ref.input_frequency
    truths = [lc.truth(kind, B, A) for _ in range(C)]
    refs = [lc.reference(kind, B, A) for _ in range(C)]
    worst = {"default vs truth": 0.0, "plain vs truth": 0.0, "default vs plain": 0.0, "default vs oracle": 0.0,
             "unlinked vs truth": 0.0}
    same_bits = []                  # per buffer: is the audio behind the complex hand-over bit-identical to the default's?
    for buf in range(lc.BUFFERS):
        st = [lc.station(kind, B, A, lc.station_index(buf, r)) for r in range(C)]
        x = se.wideband_from(st, N, ref.input_frequency, centres, B)
        ref.load(x)
        got, ran = [], []
        for t in tuners:
            t.load(x)
            with _Profile() as stages:
                got.append(t.run_all(chunk=chunk))
            ran.append({k: v for k, v in stages.items() if v})
            assert got[-1].shape == (C, A, ch)
        same_bits.append(bool(np.array_equal(got[0], got[2])))
        for i in range(C):
            iq = ref.run_pruned(i)
            want = truths[i].run(iq)
            worst["unlinked vs truth"] = max(worst["unlinked vs truth"], rel_err(got[2][i], want))
            worst["default vs truth"] = max(worst["default vs truth"], rel_err(got[0][i], want))
            worst["plain vs truth"] = max(worst["plain vs truth"], rel_err(got[1][i], want))
            worst["default vs plain"] = max(worst["default vs plain"], rel_err(got[0][i], got[1][i]))
            worst["default vs oracle"] = max(worst["default vs oracle"], rel_err(got[0][i], refs[i].run(iq)))
    linked = _option(tuners[0], hip.RCFM_OPT_PHASE_LINK)
    blocked = _option(tuners[0], hip.RCFM_OPT_PILOT_BLOCKED) if kind == "WBFM" else None
    capable = lc.phase_capable(kind, B, _planned(B))
    print("%s %d -> %d through the Tuner: %s (bound %.2e), phase link switch %s, phase capable %s, pilot blocked %s, "
          "unlinked audio bit-identical per buffer %s\n   default  %s\n   plain    %s\n   unlinked %s"
          % (kind, B, A, {k: "%.2e" % v for k, v in worst.items()}, bound, linked, capable, blocked, same_bits,
             ran[0], ran[1], ran[2]))
    # The switches (rcfm_demod_get_option returns RCFM_OPT_PHASE_LINK as set, not whether the link was taken) ...
    assert linked == 1 and _option(tuners[1], hip.RCFM_OPT_PHASE_LINK) == 0 and _option(tuners[2], hip.RCFM_OPT_PHASE_LINK) == 0
    assert _option(tuners[1], hip.RCFM_OPT_FUSED_TILES) == 0 and _option(tuners[2], hip.RCFM_OPT_FUSED_TILES) == 1
    # ... and whether the link was taken: demod.hip's phase_capable() restated from the plan must say what the table
    # says, and the audio must show it -- the third tuner differs from the default in the hand-over alone (same
    # switches otherwise, the same effective layout, the same stages apart from the discriminator / envelope kernel),
    # so its audio differs in rounding exactly where the default took phases (envelopes) and is bit-identical where not
    assert capable == lc.TUNER_PHASE_LINK[(kind, B, A)], (kind, B, A, capable)
    assert same_bits == [not capable] * lc.BUFFERS, (capable, same_bits)
    first = None if kind == "WBFM" else "envelope" if kind == "AM" else "discriminator"
    assert {k: v for k, v in ran[2].items() if k != first} == ran[0], (ran[0], ran[2])
    if kind == "WBFM":
        assert all(r["pilot_stage"] == 2 for r in ran), ran                            # chunks of 2 + 1
        assert _option(tuners[1], hip.RCFM_OPT_PILOT_BLOCKED) == 0
        assert _option(tuners[2], hip.RCFM_OPT_PILOT_BLOCKED) == blocked
        # the effective layout decides which k_pilot_stage_h40 runs: tile-blocked, it owns whole rows and the branch
        # "the channel ends inside this thread's run" is never taken.  B % 4 != 0 has no such layout; 62 500 = 250 x 250
        # has none either (rows of 250 samples are no whole quads), which is what makes it the ragged-end case
        assert blocked == 0, (B, blocked)
        assert lc.pilot_kernel(kind, B, blocked) == lc.CASES[(kind, B, A)][2]
    else:
        assert ran[0].get(first, 0) == 0 and ran[1].get(first, 0) == 2 and ran[2].get(first, 0) == 2, ran
    assert _resample_site(kind, "engine", ran[0]) == lc.resample_site(kind, B, A), ran[0]
    assert _resample_site(kind, "engine", ran[1]) != "decim_tile", ran[1]
    assert worst["default vs truth"] <= bound and worst["plain vs truth"] <= bound, worst
    assert worst["unlinked vs truth"] <= bound, worst
    assert worst["default vs plain"] <= bound, worst
    assert worst["default vs oracle"] <= TOL, worst
