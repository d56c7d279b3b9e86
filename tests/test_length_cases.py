"""CPU: tests/length_cases.py -- the table against the library's plans and the model against itself.

    coverage      every Decimate branch on both routes for FM / MFM and for WBFM; B % 8 == 4, B % 4 == 2 and odd B for WBFM;
                  the route of every row is what rcfm_fft_describe says about B and A
    model         Resample with nothing broken IS radiocore_oracle.Decimate; a mutant-free chain IS signal_edges.Truth
    conditioning  per case, all three stations and both buffers: the float32 restatement and the oracle lie within
                  bound / 10 of the float64 truth (the reference alone stays well inside what the device is held to), every
                  mutant lies at least 10 x bound away, the phase steps stay under STEP_CAP, and nothing is clipped -- apart
                  from the reference's own start-up: a fresh Deemphasis holds lfilter_zi, the state a unit step leaves
                  (deemphasis.py:48), so the first buffer of MFM / WBFM begins at about +1 and decays within the filter's 50
                  taps; those samples are clipped in the reference and here alike.
"""

import numpy as np
import pytest

import decim_cases as dc
import fft_model
import length_cases as lc
import radiocore_oracle as oracle
import signal_edges as se

STARTUP = 50        # samples of the first buffer that the de-emphasis' initial state reaches (51 taps)
IDS = ["%s-%d-%d" % c for c in lc.CASES]
# the conditioning test runs over the decimating tile's own table as well (tests/decim_cases.py: same stations, truth,
# mutant and bound; no row in both)
CONDITIONED = list(lc.CASES) + list(dc.CASES)


def library_route(B, A):
    """demod.hip, rcfm_demod_s::alloc: the engine serves a demodulator when it plans both lengths."""
    return "engine" if fft_model.describe(B) is not None and fft_model.describe(A) is not None else "rocfft"


def test_table_is_what_the_library_and_the_rules_say():
    for (kind, B, A), (br, route, pilot) in lc.CASES.items():
        assert br == lc.branch(B, A), (kind, B, A)
        assert pilot == lc.pilot_kernel(kind, B, blocked=(pilot == "h40_blocked")), (kind, B, A)   # (the layout: below)
        assert route == library_route(B, A), (kind, B, A, "the planner moved this length: exchange it")
        site = lc.resample_site(kind, B, A)
        if route == "rocfft" or A >= B or A % 2:             # no decimating tile can apply (fused_fft_decim_ifft_applies)
            assert site == ("ifft_load" if kind == "WBFM" and route == "engine" else "resample_kernel"), (kind, B, A)
        if kind != "AM":
            # the routing restated (decim_cases.route): the tile, its form and its two lengths are what the plans give
            r = dc.route(kind, B, A)
            took = (r.form, r.L, r.L2) if r is not None and r.form else None
            assert lc.tile_of(kind, B, A) == took, (kind, B, A, r, "the planner moved this length: exchange it")
        if kind == "WBFM":
            assert B > 2 * 19050, (B, "the pilot band-pass needs 19 050 Hz below B / 2")
            # k_pilot_stage_h40's ragged-end branch exists in its natural-order form only: a case labelled for it must
            # have a plan that PilotBlocked::plan refuses, and a case labelled tile-blocked one that it accepts
            layout = lc.blocked_layout(fft_model.describe(B)) and route == "engine"
            if pilot in ("h40", "h40_ragged") and route == "engine" and layout:
                print(kind, B, A, "has a tile-blocked layout: the pilot chain must decline B (the GPU test asserts it)")
            if pilot == "h40_ragged":
                assert not layout, (B, "the planner gives B a tile-blocked layout now: the ragged end would run nowhere")
            if pilot == "h40_blocked":
                assert layout, (B, "no tile-blocked layout for this plan")
    assert set(lc.TILE_CASES) <= set(lc.CASES) and not set(lc.CASES) & set(dc.CASES)


def test_table_covers_every_branch_route_and_pilot_kernel():
    for kinds in (("FM",), ("MFM",), ("WBFM",)):
        seen = {(v[1], v[0]) for k, v in lc.CASES.items() if k[0] in kinds}
        assert seen == {(r, b) for r in ("engine", "rocfft") for b in lc.BRANCHES}, (kinds, seen)
    am = {(v[1], v[0]) for k, v in lc.CASES.items() if k[0] == "AM"}
    assert am >= {(r, b) for r in ("engine", "rocfft") for b in ("same_even", "same_odd", "up_even", "up_odd", "down_even")}
    pilots = {(v[1], v[2]) for k, v in lc.CASES.items() if k[0] == "WBFM"}
    assert pilots >= {("engine", "h40_blocked"), ("engine", "h40_ragged"), ("engine", "generic_even"), ("engine", "generic_odd"),
                      ("rocfft", "h40_ragged"), ("rocfft", "generic_even"), ("rocfft", "generic_odd")}, pilots
    assert all(c in lc.CASES for c in lc.TUNER_CASES) and set(lc.TUNER_PHASE_LINK) == set(lc.TUNER_CASES)
    for kind, B, A in lc.TUNER_CASES:
        assert lc.TUNER_PHASE_LINK[(kind, B, A)] == lc.phase_capable(kind, B, fft_model.describe(B) is not None), (kind, B)
    # both hand-overs of WBFM, and the h40 kernel on phases at its ragged end
    assert lc.TUNER_PHASE_LINK[("WBFM", 62500, 12500)] and lc.CASES[("WBFM", 62500, 12500)][2] == "h40_ragged"
    assert not lc.TUNER_PHASE_LINK[("WBFM", 60750, 12150)] and not lc.TUNER_PHASE_LINK[("WBFM", 50625, 10125)]


@pytest.mark.parametrize("B,A", [(1000, 200), (1000, 201), (1001, 200), (1000, 1000), (1001, 1001), (200, 1000), (201, 1000)])
def test_resample_with_nothing_broken_is_the_oracles_decimate(B, A):
    x = np.random.default_rng(B + A).standard_normal(B)
    want = oracle.Decimate(B, A).run(x)
    np.testing.assert_array_equal(lc.Resample(B, A).run(x), want)
    if min(A, B) % 2 == 0:
        assert lc.distance(lc.Resample(B, A, nyq_gain=2.0).run(x), want) > 1e-5    # (white noise: 1 / n of the energy)
    else:
        np.testing.assert_array_equal(lc.Resample(B, A, nyq_gain=2.0).run(x), want)   # no bin n / 2: nothing to break
    if A == B:
        # the same-size step is the three-tap circular filter the pilot kernels evaluate
        side = 0.23 * (np.cos(np.pi / B) if B % 2 else 1.0)
        direct = 0.54 * x + side * (np.roll(x, 1) + np.roll(x, -1))
        assert lc.distance(direct, want) < 1e-13
        broken = lc.Resample(B, B, wrap=False).run(x)
        assert np.argmax(np.abs(broken - want)) in (0, B - 1) and np.count_nonzero(np.abs(broken - want) > 1e-12) == 2


def test_wbfm_chain_with_written_out_steps_is_signal_edges_truth():
    kind, B, A = "WBFM", 50625, 10125
    x = lc.signals(kind, B, A)[0][0]
    plain, parts = se.Truth(kind, B, A), se.Truth(kind, B, A)
    parts._same, parts._decimate = lc.Resample(B, B), lc.Resample(B, A)
    np.testing.assert_array_equal(parts.run(x), plain.run(x))


@pytest.mark.parametrize("kind,B,A", CONDITIONED, ids=["%s-%d-%d" % c for c in CONDITIONED])
def test_case_is_well_conditioned_and_tells_the_mutants_apart(kind, B, A):
    only = dc.MUTANT if (kind, B, A) in dc.CASES else None          # (decim_cases.bound: the tile's own rule alone)
    bound = lc.bound(kind, B, A, only)
    assert 0 < bound <= lc.TOL
    want = lc.truths(kind, B, A)
    low = [lc.ref32(kind, B, A) for _ in range(lc.ROWS)]
    ref = [lc.reference(kind, B, A) for _ in range(lc.ROWS)]
    full = [lc.truth(kind, B, A) for _ in range(lc.ROWS)]
    worst32 = worst_ref = step = 0.0
    for buf, x in enumerate(lc.signals(kind, B, A)):
        for r in range(lc.ROWS):
            a32 = low[r].run(x[r])
            assert a32.dtype == np.float32
            worst32 = max(worst32, lc.distance(a32, want[buf][r]))
            worst_ref = max(worst_ref, lc.distance(ref[r].run(x[r]), want[buf][r]))
            np.testing.assert_array_equal(full[r].run(x[r]), want[buf][r])
            if kind != "AM":
                step = max(step, float(np.max(np.abs(se.steps(x[r])))))
            if kind != "FM":
                raw = np.abs(full[r].unclipped)
                skip = STARTUP if (buf == 0 and kind != "AM") else 0
                assert np.max(raw[skip:]) < lc.CLIP, (kind, B, A, buf, r, float(np.max(raw[skip:])))
    dist = {k: v for k, v in lc.mutant_distances(kind, B, A).items() if only in (None, k)}
    print("%s %d -> %d: bound %.2e  ref32 %.2e  oracle %.2e  max step %.3f  mutants %s"
          % (kind, B, A, bound, worst32, worst_ref, step, {k: ["%.1e" % v for v in vs] for k, vs in dist.items()}))
    assert worst32 <= bound / 10 and worst_ref <= bound / 10, (worst32, worst_ref, bound)
    assert step <= lc.STEP_CAP, step
    if "even" in lc.branch(B, A):
        assert any(k.startswith("n/2") for k in dist), dist
    if kind == "WBFM" and only is None:
        assert "same-size step without its wrap" in dist
    # (bound = min(TOL, smallest distance / 10): this holds by construction and only guards bound()'s own arithmetic; the
    #  checks that can fail are the two above -- the reference within bound / 10, and the mutants being there at all)
    for name, per_signal in dist.items():
        assert len(per_signal) == lc.ROWS * lc.BUFFERS
        assert min(per_signal) >= 10 * bound * (1 - 1e-12), (name, per_signal, bound)
