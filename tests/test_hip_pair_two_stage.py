"""The pair FFT tile with its mono samples fetched late and its 480 / 500-point transforms in two LDS stages
(fft_kernel.h, k_fft_tile2_pair: pair_late_fetch, RCFM_PAIR_FORM).

One inverse transform carries the pilots of TWO channels; the kernel splits each of its values into the two members'
38 kHz carriers s2_0, s2_1 from the pilot bands alone, then finishes each member as m_c +- (s2_c m_c) 1.0175 with that
member's own mono sample: member 0's is fetched after the split (late), member 1's while member 0 transforms.  What can go
wrong there is an exchange: m0 / m1, s2_0 / s2_1, or a member-0 value built from member 1's mono sample.  So the two
members of a pair must differ in mono content, in L - R content and in pilot phase; test_input_conditioning pins on the
oracle's chain, without a GPU, that each of those exchanges moves the truth of both members by more than 10 TOL.

Geometry: the demodulator alone (rcfm_demod_run on channel samples, no tuner).  B = 240 000 -> A = 48 000 is 480 x 500
(pair tile <480>), B = 250 000 -> A = 50 000 is 500 x 500 (pair tile <500>): one row of 32 (16-line) / 63 (8-line) tiles per
pair, the smallest launch that reaches each kernel.  C = 1 (a pair with one member), 2 (a full pair), 3 (a pair plus an odd
one), both tile widths (RCFM_OPT_NARROW_TILES 0 / 2), at 240 000 the tile-blocked hand-over of m and p on and off
(RCFM_OPT_PILOT_BLOCKED), two consecutive buffers so that the de-emphasis state crosses.

Checks, per case, tile width, layout, buffer and channel:
    fused route   vs signal_edges.Truth (the oracle's chain on the float64 discriminator)      <= TOL = 1e-4 of peak
    fused route   vs the unfused pilot route (RCFM_OPT_PILOT_CHAIN = 0 on a second handle)      <= 4 x the unfused route's
                  own distance from the truth on that channel and buffer (both printed)
and the stage profile says which route ran (the pilot chain and the decimating tile leave no separate ifft_A; the effective
RCFM_OPT_PILOT_BLOCKED says that the chain accepts the geometry).
Measured on an MI355X over all 72 (case, width, layout, buffer, channel) rows: fused vs truth <= 3.5e-6, unfused vs truth
<= 1.3e-6, fused vs unfused <= 2.5e-6 against bounds of 4.1e-7 .. 4.9e-6: at most 0.51 of the bound.  The form before
(early fetch, 480 = 10 x 8 x 6, 500 = 10 x 10 x 5) on the same rows: fused vs truth <= 3.0e-6, fused vs unfused <= 1.9e-6,
at most 0.38 of the bound; the late fetch at those radices is bit-identical to it.
"""

import ctypes
import functools

import numpy as np
import pytest

import primitives_model as pm
import signal_edges as se
from conftest import TOL, have_gpu, rel_err

GEOMETRIES = {240_000: (48_000, [480, 500]), 250_000: (50_000, [500, 500])}   # B -> (A, pass lengths of the B-point plan)
CASES = [(B, C) for B in GEOMETRIES for C in (1, 2, 3)]
BUFFERS = 2
PILOT_PHASES = (0.4, 1.9, -1.1)     # rad, per channel: sin(2 phi) = 0.72, -0.61, -0.81
RCFM_WBFM = 2


def station(i, c, B):
    """Stereo station i of channel c, complex64 [B]: mono tones of 0.06, a 0.1 pilot at 19 kHz with phase PILOT_PHASES[c],
    L - R tones of 0.06 on the 38 kHz subcarrier locked to that pilot.  Tone frequencies and phases are drawn per station
    (signal_edges' construction: integer-Hz components, the buffer closes on itself)."""
    rng = np.random.default_rng(7000 + i)
    t = np.arange(B, dtype=np.float64) / B
    k = i % 89
    pilot = 2 * np.pi * 19000 * t + PILOT_PHASES[c]
    m = se._tones(rng, t, (300 + 7 * k, 700 + 3 * k, 1100 + k), 0.06)
    m += 0.1 * np.sin(pilot) + se._tones(rng, t, (440 + 29 * k, 1500 + 7 * k), 0.06) * np.sin(2 * pilot)
    assert np.max(np.abs(m)) <= se.STEP_BOUND
    return se._iq(m).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def signals(B):
    """[buffer] -> complex64 [3, B]; the cases with fewer channels take the first C."""
    return [np.stack([station(5 * c + 23 * buf, c, B) for c in range(3)]) for buf in range(BUFFERS)]


def _parts(chain, iq):
    """(m, s2) of signal_edges.Truth's WBFM chain: the mono signal and the 38 kHz carrier (wbfm.py:66-83)."""
    m = chain._same.run(se.steps(iq))
    chain._pll.step(chain._pilot.run(m))
    return m, chain._pll.image(2)


def _finish(chain, m, s2):
    """Truth.run from the stereo mix on (wbfm.py:86-100), mean subtracted, clipped: [A, 2]."""
    lmr = (s2 * m) * 1.0175
    l = chain._deemph[0].run(chain._decimate.run(m + lmr))
    r = chain._deemph[1].run(chain._decimate.run(m - lmr))
    lr = np.dstack((l, r))
    return np.clip(lr - np.mean(lr), -se.CLIP, se.CLIP)[0]


def exchanged(B, how):
    """[buffer][member] -> audio of the first pair's members with the stereo mix's inputs exchanged between them:
    how(m, s2, c) -> (mono, carrier) that member c's mix uses, m and s2 being the two members' lists."""
    A = GEOMETRIES[B][0]
    chains = [se.Truth("WBFM", B, A) for _ in range(2)]
    out = []
    for buf in range(BUFFERS):
        ms = [_parts(chains[c], signals(B)[buf][c]) for c in range(2)]
        m, s2 = [x[0] for x in ms], [x[1] for x in ms]
        out.append([_finish(chains[c], *how(m, s2, c)) for c in range(2)])
    return out


@functools.lru_cache(maxsize=None)
def truth(B):
    """[buffer][channel] -> audio [A, 2] of signal_edges.Truth."""
    A = GEOMETRIES[B][0]
    chains = [se.Truth("WBFM", B, A) for _ in range(3)]
    return [[chains[c].run(signals(B)[buf][c]) for c in range(3)] for buf in range(BUFFERS)]


# ---- CPU: the input tells the two members of a pair apart --------------------------------------------------------------

EXCHANGES = {
    "m0 <-> m1": lambda m, s2, c: (m[1 - c], s2[c]),
    "s2_0 <-> s2_1": lambda m, s2, c: (m[c], s2[1 - c]),
    "member 0 from m1": lambda m, s2, c: (m[1], s2[c]),
}


@pytest.mark.parametrize("B", list(GEOMETRIES))
def test_input_conditioning(B):
    """On the oracle's chain: the exchange-free evaluation of the helpers above IS signal_edges.Truth, and each exchange
    moves the audio of every member it touches, in every buffer, by more than 10 TOL of its peak ("member 0 from m1"
    leaves member 1 as it is; the odd channel of C = 3 has no partner: the kernel then reads member 0's inputs twice)."""
    base = truth(B)
    same = exchanged(B, lambda m, s2, c: (m[c], s2[c]))
    for buf in range(BUFFERS):
        for c in range(2):
            np.testing.assert_array_equal(same[buf][c], base[buf][c])
    for name, how in EXCHANGES.items():
        moved = exchanged(B, how)
        for buf in range(BUFFERS):
            for c in range(2):
                a = base[buf][c]
                d = float(np.max(np.abs(moved[buf][c] - a))) / float(np.max(np.abs(a)))
                print(B, name, "buffer", buf, "member", c, "moved %.2e of peak" % d)
                if name == "member 0 from m1" and c == 1:
                    assert d == 0.0
                else:
                    assert d > 10 * TOL, (B, name, buf, c, d)


# ---- GPU -----------------------------------------------------------------------------------------------------------------

def _run(hip, lib, B, C, narrow, blocked, chain):
    """([per buffer: audio [C, A, 2]], stage launches of the last buffer, effective RCFM_OPT_PILOT_BLOCKED)."""
    import torch
    from test_hip_am import _Profile
    A = GEOMETRIES[B][0]
    h = ctypes.c_void_p()
    hip.check(lib.rcfm_demod_create(RCFM_WBFM, C, B, A, 75e-6, 0, ctypes.byref(h)))
    try:
        hip.check(lib.rcfm_demod_set_option(h, hip.RCFM_OPT_NARROW_TILES, narrow))
        hip.check(lib.rcfm_demod_set_option(h, hip.RCFM_OPT_PILOT_BLOCKED, int(blocked)))
        if not chain:
            hip.check(lib.rcfm_demod_set_option(h, hip.RCFM_OPT_PILOT_CHAIN, 0))
        effective = ctypes.c_int(-1)
        hip.check(lib.rcfm_demod_get_option(h, hip.RCFM_OPT_PILOT_BLOCKED, ctypes.byref(effective)))
        out, ran = [], {}
        for b in range(BUFFERS):
            x = torch.from_numpy(signals(B)[b][:C].copy()).cuda()
            audio = torch.empty((C, A, 2), dtype=torch.float32, device="cuda")

            def go():
                hip.check(lib.rcfm_demod_run(h, 0, C, hip.ptr(x), hip.ptr(audio), hip.stream()))
                torch.cuda.synchronize()

            if b == BUFFERS - 1:
                with _Profile() as ran:
                    go()
            else:
                go()
            out.append(audio.cpu().numpy())
        return out, {k: v for k, v in ran.items() if v}, effective.value
    finally:
        hip.check(lib.rcfm_demod_destroy(h))


@pytest.mark.parametrize("B,C", CASES, ids=["%d-%d" % c for c in CASES])
@pytest.mark.gpu
@pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")
def test_pair_tile(B, C):
    import radiocore as rc
    from radiocore._internal import hip
    assert rc.HasCuda(), "librcfm.so did not load or sees no device"
    hip.torch()
    lib = hip.lib()
    plan = hip.FftPlan()
    hip.check(lib.rcfm_fft_describe(B, 0, ctypes.byref(plan)))
    lengths = sorted(plan.passes[i].L for i in range(plan.npass))
    assert lengths == GEOMETRIES[B][1], (B, lengths)     # the pair tile of this length is the one that runs
    want = truth(B)
    for narrow in (0, 2):
        plain, ran_p, eff_p = _run(hip, lib, B, C, narrow, True, False)
        assert eff_p == 0 and ran_p.get("ifft_A", 0) >= 1, (ran_p, eff_p)
        for blocked in ((1, 0) if B == 240_000 else (1,)):
            fused, ran_f, eff_f = _run(hip, lib, B, C, narrow, blocked, True)
            print(B, C, "narrow_tiles", narrow, "blocked", blocked, "fused stages", ran_f, "unfused stages", ran_p)
            assert eff_f == blocked, (B, C, narrow, blocked, eff_f)   # on: the chain accepts this geometry and layout
            assert all(ran_f.get(k, 0) >= 1 for k in ("rfft_B", "ifft_B", "fft_B")) and "ifft_A" not in ran_f, ran_f
            for b in range(BUFFERS):
                for i in range(C):
                    ref = want[b][i]
                    e_f, e_p = pm.worst_row(fused[b][i][None], ref[None]), pm.worst_row(plain[b][i][None], ref[None])
                    e_r = rel_err(fused[b][i], plain[b][i])
                    print("   buffer %d channel %d: fused vs truth %.2e  unfused vs truth %.2e  fused vs unfused %.2e (bound %.2e)"
                          % (b, i, e_f, e_p, e_r, 4 * e_p))
                    assert e_f <= TOL, (B, C, narrow, blocked, b, i, e_f)
                    assert e_r <= 4 * e_p, (B, C, narrow, blocked, b, i, e_r, e_p)
