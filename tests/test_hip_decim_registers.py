"""The decimating FFT tile's register form (fft_kernel.h, k_fft_tile2_decim with REG: 500 -> 100 as 4 x 5 x 5).

After transform 1's last stage thread (g, lane) holds the four surviving rows g, g + 25, g + 50, g + 75 of the short
spectrum; weight, Nyquist merge (Y[A/2] = X[A/2] + X[-A/2]), the DC hook, the re/im swap and the radix-4 first stage of
IFFT_A run from those registers.  The merge and the DC hook both live in ONE lane (g = 0, line 0) of ONE tile per
signal, so the input must make them matter: every station's modulation carries a DC level (a carrier LEVEL * B / 2 Hz off
centre) and a tone at exactly A / 2 = 24 kHz.  test_input_conditioning pins that on the oracle, without a GPU: dropping
bin A/2 or the DC term moves the audio by more than 10 TOL, so the GPU test cannot pass with either lost.

Geometry: B = 240 000 -> A = 48 000 is 480 x 500 -> 480 x 100: one row of 30 (16-line) or 60 (8-line) tiles per signal,
the smallest launch that reaches the kernel.  WBFM at C = 1 and 3 (one complex signal per channel), MFM and FM at C = 2
and 3 (two channels per complex signal: a full pair, and a pair plus an odd one out), both tile widths
(set_kernel_options(narrow_tiles = 0 / 2): at these channel counts the default would pick the 8-line build only, the
benchmark runs the 16-line one), two consecutive buffers so that the de-emphasis state crosses.

Checks, per case, tile width, buffer and channel:
    fused route   vs signal_edges.Truth (the oracle's chain on the float64 discriminator)      <= TOL = 1e-4 of peak
    fused route   vs the unfused route (RCFM_OPT_DECIM_TILE off: separate resample, 10 x 10)   <= 4 x the unfused route's
                  own distance from the truth on that channel and buffer (both printed)
and the stage profile says which route ran.  Measured on an MI355X over all 56 (case, width, buffer, channel) rows: fused
vs truth <= 1.2e-6, unfused vs truth <= 1.3e-6, fused vs unfused <= 5.2e-7 against bounds of 4.0e-7 .. 5.0e-6 (at most
0.23 of the bound); the 4 x 25 form of the short plan (-DRCFM_DECIM_100=4,25,1) passes the same checks (<= 0.45).
"""

import functools

import numpy as np
import pytest

import primitives_model as pm
import radiocore_oracle as oracle
import signal_edges as se
from conftest import TOL, have_gpu, rel_err

N, B, A = 2_400_000, 240_000, 48_000
LEVELS = (0.2, -0.2, 0.2)          # discriminator mean per channel: LEVEL * B / 2 = 24 000 Hz of carrier offset
NYQ_AMP = 0.15                     # the 24 kHz tone, in discriminator units
CASES = [("WBFM", 1), ("WBFM", 3), ("MFM", 2), ("MFM", 3), ("FM", 2), ("FM", 3)]
BUFFERS = 2


def station(i, level, stereo):
    """signal_edges.dc_station plus a tone at exactly A / 2 Hz (phase drawn per station, kept off the zero crossing at
    the audio's sampling instants: cos(pi n + phase) = +-cos(phase))."""
    rng = np.random.default_rng(6000 + i)
    t = np.arange(B, dtype=np.float64) / B
    k = i % 89
    m = np.full(B, float(level)) + se._tones(rng, t, (300 + 7 * k, 700 + 3 * k, 1100 + k), 0.06)
    m += NYQ_AMP * np.cos(2 * np.pi * (A // 2) * t + rng.uniform(-1.0, 1.0))
    if stereo:
        pilot, sub = se._stereo_parts(rng, t, k, 0.12)
        m += 0.1 * pilot + sub
    assert np.max(np.abs(m)) <= se.STEP_BOUND
    return se._iq(m)


@functools.lru_cache(maxsize=None)
def band(kind, C):
    """[per buffer: (x, [iq per channel])]: the wideband buffers and what the oracle's Tuner hands each channel."""
    ref = se.oracle_tuner(B, C, N)
    out = []
    for buf in range(BUFFERS):
        st = [station(i + 17 * buf, LEVELS[i], kind == "WBFM") for i in range(C)]
        x = se.wideband_from(st, N, ref.input_frequency, se.centres_of(B, C), B)
        ref.load(x)
        out.append((x, [ref.run_pruned(i) for i in range(C)]))
    return out


def truths(kind, C, patch=None):
    """[buffer][channel] -> (audio [A, ch], mean subtracted) of signal_edges.Truth; patch(Y) edits the spectrum that
    oracle.resample_spectrum returns for the decimation B -> A."""
    orig = oracle.resample_spectrum

    def patched(X, num, nx, real_input, W=None):
        Y = orig(X, num, nx, real_input, W)
        if num == A and nx == B:
            patch(Y)
        return Y

    chains = [se.Truth(kind, B, A) for _ in range(C)]
    out = []
    try:
        if patch is not None:
            oracle.resample_spectrum = patched
        for _, iqs in band(kind, C):
            out.append([(chains[i].run(iqs[i]), float(chains[i].mean)) for i in range(C)])
    finally:
        oracle.resample_spectrum = orig
    return out


@functools.lru_cache(maxsize=None)
def truth(kind, C):
    return truths(kind, C)


# ---- CPU: the input makes the merged Nyquist row and the DC hook matter ----------------------------------------------

@pytest.mark.parametrize("kind", ["WBFM", "MFM", "FM"])
def test_input_conditioning(kind):
    """On the oracle: with bin A/2 of the decimated spectrum zeroed the audio of every channel and buffer moves by more
    than 10 TOL of its peak; so does it (MFM, WBFM: the kinds whose tail subtracts the mean, which the device derives
    from the DC hook's bin) when the DC term is skipped, i.e. by |mean| / peak.  FM has no mean to subtract: its DC level
    stays in the audio and is covered by the parity check itself."""
    C = 1
    def zero_nyquist(Y):
        Y[A // 2] = 0.0           # real input: the half spectrum's last bin, scipy's doubled Nyquist bin
    base, cut = truth(kind, C), truths(kind, C, zero_nyquist)
    for buf in range(BUFFERS):
        (a, mean), (b, _) = base[buf][0], cut[buf][0]
        peak = float(np.max(np.abs(a)))
        moved = float(np.max(np.abs(a - b))) / peak
        print(kind, "buffer", buf, "bin A/2 zeroed: %.2e of peak" % moved, " |mean| / peak %.2e" % (abs(mean) / peak))
        assert moved > 10 * TOL, (kind, buf, moved)
        if kind != "FM":
            assert abs(mean) / peak > 10 * TOL, (kind, buf, mean, peak)
        else:
            assert abs(float(np.mean(a))) / peak > 10 * TOL, (kind, buf)


# ---- GPU -----------------------------------------------------------------------------------------------------------------

def _run(rc, kind, C, narrow, fused):
    """([per buffer: audio [C, A, ch]], stage launches of the last run_all)."""
    from radiocore._internal import hip
    from test_hip_am import _Profile
    tuner = rc.Tuner()
    for f in se.centres_of(B, C):
        tuner.add_channel(f, B, getattr(rc, kind)(B, A))
    tuner.request_bandwidth(float(N))
    tuner.set_kernel_options(narrow_tiles=narrow)
    handle = tuner._batched_demod(*tuner._plan_uniform(), 0)
    if not fused:
        hip.check(hip.lib().rcfm_demod_set_option(handle, hip.RCFM_OPT_DECIM_TILE, 0))
    out, ran = [], {}
    for b, (x, _) in enumerate(band(kind, C)):
        tuner.load(x)
        if b == BUFFERS - 1:
            with _Profile() as ran:
                audio = tuner.run_all()
        else:
            audio = tuner.run_all()
        assert audio.shape == (C, A, 2 if kind == "WBFM" else 1) and audio.dtype == np.float32
        out.append(audio)
    return out, {k: v for k, v in ran.items() if v}


@pytest.mark.parametrize("kind,C", CASES, ids=["%s-%d" % c for c in CASES])
@pytest.mark.gpu
@pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")
def test_register_decimation(kind, C):
    import radiocore as rc
    assert rc.HasCuda(), "librcfm.so did not load or sees no device"
    want = truth(kind, C)
    # the stage that only the route WITHOUT the decimating tile launches: WBFM's separate IFFT_A, FM / MFM's resample kernel
    marker = "ifft_A" if kind == "WBFM" else "audio_spectrum"
    for narrow in (0, 2):
        fused, ran_f = _run(rc, kind, C, narrow, True)
        plain, ran_p = _run(rc, kind, C, narrow, False)
        print(kind, C, "narrow_tiles", narrow, "fused stages", ran_f, "unfused stages", ran_p)
        assert marker not in ran_f and ran_p.get(marker, 0) >= 1, (ran_f, ran_p)
        for b in range(BUFFERS):
            for i in range(C):
                ref = want[b][i][0]
                e_f, e_p = pm.worst_row(fused[b][i][None], ref[None]), pm.worst_row(plain[b][i][None], ref[None])
                e_r = rel_err(fused[b][i], plain[b][i])
                print("   buffer %d channel %d: fused vs truth %.2e  unfused vs truth %.2e  fused vs unfused %.2e (bound %.2e)"
                      % (b, i, e_f, e_p, e_r, 4 * e_p))
                assert e_f <= TOL, (kind, C, narrow, b, i, e_f)
                assert e_r <= 4 * e_p, (kind, C, narrow, b, i, e_r, e_p)
