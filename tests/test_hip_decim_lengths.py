"""GPU: the decimating two-transform FFT tile at every long length and run-time radix, and WBFM's pilot-chain tiles at every
length a bandwidth reaches (tests/decim_cases.py has the routing and the table, tests/test_decim_cases.py pins both without
a GPU; stations, float64 truth and the bound are tests/length_cases.py's, conditioned by tests/test_length_cases.py).

Every station carries a tone at exactly A / 2 Hz, so bin A / 2 -- the tile's Nyquist merge, one point of one tile, and the
negative Nyquist row every line keeps -- decides whether a case passes: with "n/2 not doubled" the truth moves by at least
10 x the bound the device is held to (decim_cases.bound = min(1e-4, closest such mutant / 10)).

Per row and tile width (RCFM_OPT_NARROW_TILES 0: 16 lines, 2: 8 lines): the demodulator alone on channel samples
(rcfm_demod_run, no tuner), three stations -- FM and MFM ride two per complex signal, so one pair has a lone member --,
two consecutive buffers (de-emphasis state), three evaluations:
    default                      the tile, where decim_cases.route gives it one
    RCFM_OPT_DECIM_TILE = 0      the same chain with a separate resample
    RCFM_OPT_PILOT_CHAIN = 0     WBFM: separate transforms around the Hilbert mask and the stereo mix (and no tile either)
each against the float64 truth at the row's bound.  The stage profile of the second buffer says which ran: with the tile
FM / MFM show no audio_spectrum stage and WBFM no ifft_A stage (run_wbfm_engine has no audio_spectrum stage in any form: its
separate resample rides on IFFT_A's first pass, so ifft_A is its mark, as in tests/test_hip_lengths.py); the refused
neighbours and the option-off runs show the stage.  The fused and the unfused audio must differ somewhere (another kernel,
another rounding) where the profile does; on the refused rows the switch must change nothing, not a bit.  The audio is
written between two guard rows of a sentinel, which must survive.  WBFM: the effective RCFM_OPT_PILOT_BLOCKED is what
length_cases.blocked_layout says of the plan in the order the route runs it.

Measured on an MI355X (the table of tests/decim_cases.py has every row; both tile widths return the same bits): FM / MFM
3.4e-7 .. 7.1e-7 of peak with the tile and 3.4e-7 .. 7.3e-7 without; WBFM 3.9e-7 .. 2.3e-6 with the tile, 5.1e-7 .. 2.2e-6
without, 4.1e-7 .. 2.2e-6 without the pilot chain, and 7.2e-6 / 7.3e-6 / 5.2e-6 at 56 250 -> 16 200; bounds 4.65e-5
(40 960 -> 30 720) and 1e-4.  With the Nyquist merge taken out of k_fft_tile2_decim_rt (a scratch build) the 24 run-time
rows fail at both widths with 1.5e-3 .. 0.64 of peak; with `k >= L - L2 / 2` made `>` they fail with 2.2e-3 .. 0.81.
"""

import ctypes

import numpy as np
import pytest

import decim_cases as dc
import length_cases as lc
from conftest import have_gpu, rel_err
from test_hip_am import _Profile

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

SENTINEL = -12345.0
PARAMS = [c + (w,) for c in dc.CASES for w in (0, 2)]
IDS = ["%s-%d-%d-%s" % (k, B, A, "w16" if w == 0 else "w8") for k, B, A, w in PARAMS]


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


def _run(rc, kind, B, A, narrow, off=()):
    """([per buffer: audio [ROWS, A, ch]], stage launches of the last buffer, effective RCFM_OPT_PILOT_BLOCKED) of one
    handle with the options `off` switched off; the guard rows around the audio are checked here."""
    import torch
    from radiocore._internal import hip
    lib = hip.lib()
    ch = lc.channels(kind)
    demod = getattr(rc, kind)(B, A, batch=lc.ROWS)
    h = demod._handle.value
    hip.check(lib.rcfm_demod_set_option(h, hip.RCFM_OPT_NARROW_TILES, narrow))
    for name in off:
        hip.check(lib.rcfm_demod_set_option(h, getattr(hip, name), 0))
    blocked = ctypes.c_int(-1)
    hip.check(lib.rcfm_demod_get_option(h, hip.RCFM_OPT_PILOT_BLOCKED, ctypes.byref(blocked)))
    out, ran = [], {}
    for buf, x in enumerate(lc.signals(kind, B, A)):
        xd = torch.from_numpy(x.copy()).cuda()
        guarded = torch.full((lc.ROWS + 2, A, ch), SENTINEL, dtype=torch.float32, device="cuda")
        audio = guarded[1:lc.ROWS + 1]
        assert audio.is_contiguous()

        def go():
            hip.check(lib.rcfm_demod_run(h, 0, lc.ROWS, hip.ptr(xd), hip.ptr(audio), hip.stream()))
            torch.cuda.synchronize()

        if buf == lc.BUFFERS - 1:
            with _Profile() as ran:
                go()
        else:
            go()
        guards = guarded[[0, lc.ROWS + 1]].cpu().numpy()
        assert np.array_equal(guards, np.full_like(guards, SENTINEL)), (kind, B, A, narrow, off, buf, "wrote outside the audio")
        out.append(audio.cpu().numpy())
    return out, {k: v for k, v in ran.items() if v}, blocked.value


def _errors(kind, B, A, audio):
    want = lc.truths(kind, B, A)
    return [rel_err(audio[buf][r], want[buf][r]) for buf in range(lc.BUFFERS) for r in range(lc.ROWS)]


def _took_the_tile(kind, ran):
    """The stage profile's answer (module docstring)."""
    assert ran.get("rfft_B", 0) >= 1, ran
    if kind == "WBFM":
        assert ran.get("audio_spectrum", 0) == 0 and ran.get("pilot_stage", 0) == 1, ran
        return ran.get("ifft_A", 0) == 0
    assert ran.get("ifft_A", 0) >= 1 and ran.get("discriminator", 0) == 1, ran
    return ran.get("audio_spectrum", 0) == 0


@pytest.mark.parametrize("kind,B,A,narrow", PARAMS, ids=IDS)
def test_decimating_tile(rc, kind, B, A, narrow):
    import fft_model
    n1, L, L2, radices, form = dc.CASES[(kind, B, A)]
    r = dc.route(kind, B, A)
    assert r is not None and tuple(r[:5]) == dc.CASES[(kind, B, A)], (r, "the planner moved this length: exchange it")
    bound = dc.bound(kind, B, A)
    fused, ran_f, blocked_f = _run(rc, kind, B, A, narrow)
    plain, ran_p, blocked_p = _run(rc, kind, B, A, narrow, off=("RCFM_OPT_DECIM_TILE",))
    e_f, e_p = _errors(kind, B, A, fused), _errors(kind, B, A, plain)
    same = all(np.array_equal(a, b) for a, b in zip(fused, plain))
    print("DECIM %s %d -> %d w%d: %d x %d -> %d %s %s: bound %.2e  with the tile %.2e  without %.2e  bit-identical %s\n"
          "   default %s\n   no tile %s" % (kind, B, A, 8 if narrow else 16, n1, L, L2, radices, form, bound, max(e_f), max(e_p),
                                           same, ran_f, ran_p))
    assert _took_the_tile(kind, ran_f) == (form is not None), (kind, B, A, form, ran_f)
    assert not _took_the_tile(kind, ran_p), ran_p
    if form is None:
        # a refused neighbour: a separate resample either way, and the switch changes nothing
        assert ran_f.get("audio_spectrum", 0) >= 1 and ran_f == ran_p and same, (ran_f, ran_p, same)
    else:
        assert ran_f != ran_p and not same, (ran_f, ran_p, "RCFM_OPT_DECIM_TILE did nothing")
    assert max(e_f) <= bound, (kind, B, A, narrow, e_f, bound)
    assert max(e_p) <= bound, (kind, B, A, narrow, e_p, bound)
    if kind != "WBFM":
        assert blocked_f == 0 and blocked_p == 0
        return
    # the pilot chain ahead of the tile: k_fft_tile2<MidHilbertMask> at L points, k_fft_tile2_pair at n1 points
    assert dc.pilot_tiles_of(kind, B, A) == (L, n1)
    assert ran_f.get("hilbert_mask", 0) == 0 and ran_f.get("stereo_mix", 0) == 0 and ran_f.get("fft_B", 0) > 0, ran_f
    assert all(ran_f.get(k, 0) >= 1 for k in ("rfft_B", "ifft_B", "fft_B")), ran_f
    layout = B % 4 == 0 and lc.blocked_layout(fft_model.describe_plan(B, (n1, L)))
    assert blocked_f == blocked_p == int(layout), (B, n1, L, blocked_f, blocked_p, layout)
    loose, ran_l, blocked_l = _run(rc, kind, B, A, narrow, off=("RCFM_OPT_PILOT_CHAIN",))
    e_l = _errors(kind, B, A, loose)
    print("   no pilot chain %.2e %s" % (max(e_l), ran_l))
    assert blocked_l == 0 and not _took_the_tile(kind, ran_l), (blocked_l, ran_l)
    assert ran_l != ran_f and not all(np.array_equal(a, b) for a, b in zip(fused, loose)), "RCFM_OPT_PILOT_CHAIN did nothing"
    assert max(e_l) <= bound, (kind, B, A, narrow, e_l, bound)
