"""GPU: the tone bank (rcfm_tone_bank_run), the tone score (rcfm_tone_score) and the tone squelch through the Tuner, against
the definition in include/rcfm.h evaluated in float64 by tests/tone_model.py.

Accuracy.  err = max |P_got - P_model| / (sum_i |w_i x_i| / S)^2 over channels, frames and tones, for each of the two inputs
of a shape (noise plus tones, pure noise) on its own: the denominator is the largest value P can take for that frame.
Bounds, per input: at most 4 x the float32 yardstick's err on the same input (tone_model.tone_bank_f32: float32 tables, products and numpy float32 sums --
the margin test_hip_tuner_gather.py gives a device sum of another order), and never above 1e-4.  E: the relative error
within 4 x the yardstick's.  Every case prints its figures.
"""

import ctypes
import importlib.util
import os

import numpy as np
import pytest

import squelch_model
import tone_model
import workloads
from conftest import ROOT, have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

CEILING = 1e-4


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def oracle():
    import radiocore_oracle
    return radiocore_oracle


class Bank:
    """A device tone bank made straight through the ABI: nu in cycles per sample."""

    def __init__(self, nu, L, window=None):
        from radiocore._internal import hip
        self.hip, self.lib = hip, hip.lib()
        self.nu = np.ascontiguousarray(nu, dtype=np.float64)
        self.L, self.K = int(L), len(self.nu)
        self.window = None if window is None else np.ascontiguousarray(window, dtype=np.float32)
        h = ctypes.c_void_p()
        hip.check(self.lib.rcfm_tone_bank_create(self.K, self.nu.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.L,
                                                 self.window.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
                                                 if self.window is not None else None, ctypes.byref(h)))
        self.handle = hip.Handle(h, self.lib.rcfm_tone_bank_destroy)

    def run(self, audio, step=1, offset=0, energy=True):
        """audio: device tensor [count, A step] -> numpy (P [count, F, K], E [count, F] or None), on the current stream."""
        import torch
        hip = self.hip
        count, A = int(audio.shape[0]), int(audio.shape[1]) // step
        F = A // self.L
        P = torch.full((count, F, self.K), -1.0, dtype=torch.float32, device="cuda")
        E = torch.full((count, F), -1.0, dtype=torch.float32, device="cuda") if energy else None
        hip.check(self.lib.rcfm_tone_bank_run(self.handle.value, hip.ptr(audio), count, A, step, offset, hip.ptr(P),
                                              hip.ptr(E) if energy else None, hip.stream()))
        torch.cuda.current_stream().synchronize()
        return P.cpu().numpy(), (E.cpu().numpy() if energy else None)


def _nu(K, seed):
    """K frequencies in [0, 0.5]; both ends are among them from K = 3 on."""
    nu = np.sort(np.random.default_rng(seed).uniform(0.0, 0.5, K))
    if K >= 3:
        nu[0], nu[-1] = 0.0, 0.5
    return nu


def _window(kind, L, seed):
    if kind == "hann":
        return tone_model.hann(L)
    if kind == "random":                 # asymmetric, with negative values, sum > 0
        return (np.random.default_rng(seed).uniform(-0.2, 1.0, L)).astype(np.float32)
    return None


def _inputs(count, A, step, nu, seed):
    """Two float32 [count, A step] inputs: noise plus sinusoids (two at tones of the bank, one between two tones), and
    pure noise.  With step = 2 the other side of each row holds something else entirely."""
    rng = np.random.default_rng(seed)
    n = np.arange(A, dtype=np.float64)
    out = []
    for with_tones in (True, False):
        x = 0.2 * rng.standard_normal((count, A * step))
        if with_tones:
            side = x[:, ::step] if step > 1 else x
            for c in range(count):
                for f, a in ((nu[c % len(nu)], 0.1), (nu[(3 * c + 1) % len(nu)], 0.03), (0.1937 + 0.01 * c, 0.05)):
                    side[c] += a * np.cos(2 * np.pi * f * n + 0.3 * c)
        out.append(x.astype(np.float32))
    return out


#        A      L      K   count step offset window
SHAPES = [
    (1000,   160,   39, 1, 1, 0, "hann"),        # six short frames and a tail of 40 samples
    (1000,   160,   1,  5, 1, 0, None),          # one tone: a single wave
    (1000,   1000,  64, 5, 1, 0, "random"),      # eight waves, the last chunk of a frame partly filled (1000 = 62 x 16 + 8)
    (7875,   1000,  39, 5, 1, 0, "hann"),        # odd A: every other row is unaligned, and frames inside a row too
    (8000,   8000,  39, 5, 1, 0, "hann"),        # the CTCSS bank over a whole row: 500 chunks, eight per lane
    (8000,   8000,  64, 1, 1, 0, None),
    (8000,   1,     39, 5, 1, 0, None),          # frames of one sample: P = x^2 for every tone
    (20000,  9000,  39, 2, 1, 0, "random"),      # two frames of two segments each (8192 + 808) and a tail
    (48000,  48000, 39, 2, 1, 0, "hann"),        # six segments (the last 7040 samples) and the finish step
    (48000,  48000, 64, 2, 1, 0, "random"),
    (1000,   160,   39, 5, 2, 0, "hann"),        # one side of interleaved stereo: 4-byte loads
    (8000,   8000,  16, 5, 2, 1, None),
    (20000,  9000,  5,  2, 2, 1, "hann"),
]


@pytest.mark.parametrize("A,L,K,count,step,offset,window", SHAPES)
def test_tone_bank_against_the_model(rc, A, L, K, count, step, offset, window):
    import torch
    nu = _nu(K, seed=A + L + K)
    w = _window(window, L, seed=L)
    bank = Bank(nu, L, w)
    missed = []
    for name, x in zip(("noise plus tones", "pure noise"), _inputs(count, A, step, nu, seed=A * 7 + K)):
        P, E = bank.run(torch.from_numpy(x).cuda(), step, offset)
        Pm, Em = tone_model.tone_bank(x, nu, L, w, step, offset)
        Py, Ey = tone_model.tone_bank_f32(x, nu, L, w, step, offset)
        assert P.dtype == np.float32 and P.shape == Pm.shape and E.shape == Em.shape
        top = tone_model.largest_power(x, L, w, step, offset)[..., None]
        err = float(np.max(np.abs(P - Pm) / top))
        yerr = float(np.max(np.abs(Py - Pm) / top))
        e_rel = float(np.max(np.abs(E - Em) / Em))
        ye_rel = float(np.max(np.abs(Ey - Em) / Em))
        print("A=%d L=%d K=%d count=%d step=%d offset=%d window=%s, %s: P err %.3g (yardstick %.3g, bound %.3g), E rel %.3g "
              "(yardstick %.3g, bound %.3g)" % (A, L, K, count, step, offset, window, name, err, yerr, min(4 * yerr, CEILING),
                                                e_rel, ye_rel, 4 * ye_rel))
        # every input is held to its own yardstick; the figures of both are printed before anything is asserted
        if not err <= CEILING:
            missed.append((name, "P above the ceiling", err))
        if not err <= 4 * yerr:
            missed.append((name, "P", err, yerr))
        if not e_rel <= 4 * ye_rel:
            missed.append((name, "E", e_rel, ye_rel))
    assert not missed, missed


def test_a_sinusoid_at_a_tone_reads_a_squared_over_four(rc):
    """Through radiocore.ToneBank (frequencies in Hz, nu = f / A): amplitude 0.3 at each of three CTCSS tones -- 67.0, 88.5
    and 100.0 Hz, whose doubles are whole cycles per buffer, so the mirror term vanishes for the rect window too."""
    import torch
    from radiocore.tools import tones
    A, a = 8000, 0.3
    for window in ("hann", "rect"):
        bank = rc.ToneBank(tones.CTCSS, window=window)
        x = np.stack([tone_model.tone(A, tones.CTCSS[k], a, 0.4 * k) for k in (0, 8, 12)]).astype(np.float32)
        P, E = bank.run(torch.from_numpy(x).cuda())
        P, E = P.cpu().numpy(), E.cpu().numpy()
        assert P.shape == (3, 1, 39) and E.shape == (3, 1)
        for c, k in enumerate((0, 8, 12)):
            assert abs(P[c, 0, k] - a * a / 4) <= 1e-5 * a * a, (window, k, P[c, 0, k])
        assert np.allclose(E, a * a / 2, rtol=1e-5)
    with pytest.raises(ValueError):                      # A < L
        rc.ToneBank([100.0], frame=9000).run(torch.zeros(1, 8000, device="cuda"))
    short = Bank(_nu(3, seed=1), 2000)                   # ... and through the ABI: RCFM_ERR_SIZE, nothing launched
    x, P = torch.zeros(1, 1999, device="cuda"), torch.full((1, 1, 3), -1.0, device="cuda")
    assert short.lib.rcfm_tone_bank_run(short.handle.value, short.hip.ptr(x), 1, 1999, 1, 0, short.hip.ptr(P), None,
                                        short.hip.stream()) == -1
    torch.cuda.synchronize()
    assert (P.cpu().numpy() == -1.0).all()
    with pytest.raises(ValueError):                      # a tone above half the audio rate
        rc.ToneBank([5000.0]).run(torch.zeros(1, 8000, device="cuda"))


@pytest.mark.parametrize("A,L,K", [(7875, 1000, 39), (20000, 9000, 64)])
def test_bit_identity(rc, A, L, K):
    """A second run, a run on a second stream, channels [2, 5) alone and energy = NULL: the same bits."""
    import torch
    nu = _nu(K, seed=5)
    bank = Bank(nu, L, _window("random", L, seed=6))
    x = torch.from_numpy(_inputs(5, A, 1, nu, seed=9)[0]).cuda()
    P, E = bank.run(x)
    P2, E2 = bank.run(x)
    assert np.array_equal(P, P2) and np.array_equal(E, E2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        P3, E3 = bank.run(x)
    assert np.array_equal(P, P3) and np.array_equal(E, E3)
    P4, E4 = bank.run(x[2:5])                              # odd A: the sub-range starts at another alignment
    assert np.array_equal(P[2:5], P4) and np.array_equal(E[2:5], E4)
    P5, none = bank.run(x, energy=False)
    assert none is None and np.array_equal(P, P5)
    assert (P >= 0).all() and (E > 0).all()                # and every element was written (the outputs start at -1)


def _check_squelched(got, base, mask, what):
    for i, is_open in enumerate(mask):
        if is_open:
            assert np.array_equal(got[i].view(np.uint32), base[i].view(np.uint32)), (what, "open row changed", i)
        else:
            assert np.array_equal(got[i].view(np.uint32), np.zeros_like(got[i], np.uint32)), (what, "closed row is not zero", i)


def test_tone_score_and_squelch_against_the_model(rc):
    """rcfm_tone_score on a bank's own output: +inf and NaN exactly, everything else within 1e-5; then through
    rcfm_squelch with thresholds at least 3 x away from every model score."""
    import torch
    from radiocore._internal import hip
    from radiocore.tools import tones
    lib = hip.lib()
    A, L, C = 8000, 2000, 12
    nu = np.array(tones.CTCSS) / A
    rng = np.random.default_rng(21)
    x = np.zeros((C, A))
    carried = [0, 5, 5, 12, 38, 20, 7, 7, 30, 1, 2, 3]
    for c in range(C):
        x[c] = tone_model.speech(rng, A) + tone_model.tone(A, tones.CTCSS[carried[c]], 0.15, 0.5 * c)
    x[9] = 0.0                                             # a silent channel: E == 0 in every frame
    x[10, :2 * L] = 0.0                                    # ... and one that is silent in two of its four frames
    x = x.astype(np.float32)
    bank = Bank(nu, L, tone_model.hann(L))
    xd = torch.from_numpy(x).cuda()
    P, E = bank.run(xd)
    want = np.array([0, 5, 20, -1, 38, 30, 7, -1, 30, 1, 2, 39], np.int32)     # 39 is outside the bank: NaN by definition
    gate = np.array([1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1], np.uint8)
    model = {g is not None: tone_model.tone_score(*tone_model.tone_bank(x, nu, L, tone_model.hann(L)), want, g) for g in (None, gate)}
    Pd, Ed, wd, gd = (torch.from_numpy(a).cuda() for a in (P, E, want, gate))
    for gated in (False, True):
        score = torch.full((C,), -7.0, dtype=torch.float32, device="cuda")
        hip.check(lib.rcfm_tone_score(hip.ptr(Pd), hip.ptr(Ed), hip.ptr(wd), hip.ptr(gd) if gated else None, C, A // L, 39,
                                      hip.ptr(score), hip.stream()))
        got, exp = score.cpu().numpy(), model[gated]
        print("gate %s: score %s" % (gated, np.array2string(got, precision=4)))
        special = ~np.isfinite(exp)
        assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isposinf(got), np.isposinf(exp))
        assert np.allclose(got[~special], exp[~special], rtol=1e-5, atol=0)
        assert got[9] == 0.0 and exp[9] == 0.0
        ratio = np.full(C, 0.02, np.float32)
        assert tone_model.margin(exp, ratio) >= 3.0, tone_model.margin(exp, ratio)
        mask_model = tone_model.open_mask(exp, ratio)
        audio = xd.clone()
        mask = torch.full((C,), 9, dtype=torch.uint8, device="cuda")
        hip.check(lib.rcfm_squelch(hip.ptr(score), hip.ptr(torch.from_numpy(ratio).cuda()), C, A, hip.ptr(audio),
                                   hip.ptr(mask), hip.stream()))
        assert np.array_equal(mask.cpu().numpy().astype(bool), mask_model)
        _check_squelched(audio.cpu().numpy(), x, mask_model, "gated" if gated else "plain")
    assert model[False].tolist()[3] == np.inf and mask_model.tolist() == [True, True, False, True, False, False, True, False,
                                                                         True, False, True, False]   # (the gated pass)


# ---- through the Tuner ---------------------------------------------------------------------------------------------

N, B, AUDIO, C = 1_000_000, 25000, 8000, 24
RATIO = 0.01


def _fm_station(rng, B, tone_hz, level):
    """Narrow FM at the channel rate: noise-like speech (300 .. 3000 Hz, sigma 0.2) plus a CTCSS tone of amplitude 0.1."""
    S = np.fft.rfft(rng.standard_normal(B))
    f = np.fft.rfftfreq(B, 1.0 / B)
    S[(f < 300.0) | (f > 3000.0)] = 0.0
    s = np.fft.irfft(S, B)
    m = 0.2 * s / np.std(s) + 0.1 * np.cos(2 * np.pi * tone_hz * np.arange(B) / B + rng.uniform(0, 6.28))
    return level * np.exp(2j * np.pi * 0.2 * np.cumsum(m))


def _tuner(rc, kind="FM", bw=B, A=AUDIO, channels=C, n=N):
    centres = workloads.channel_grid(channels, bw)
    t = rc.Tuner()
    for f in centres:
        t.add_channel(f, bw, getattr(rc, kind)(bw, A))
    t.request_bandwidth(float(n))
    return t, centres


@pytest.fixture(scope="module")
def fm_band(rc, oracle):
    """Two buffers of the 24-channel narrow-FM band, stations with CTCSS tones on some channels at levels 20 dB apart, the
    level model's thresholds (10 dB over the floor, >= 3 dB from every level) and masks -- computed once."""
    from radiocore.tools import tones
    t, centres = _tuner(rc)
    ref = oracle.Tuner()
    for f in centres:
        ref.add_channel(f, B, None)
    ref.request_bandwidth(float(N))
    plans = ({1: 8, 4: 8, 9: 20, 15: 8, 22: 38}, {1: 20, 2: 8, 9: 8, 15: 8, 23: 0})      # channel -> CTCSS index
    bufs, level_masks, thr = [], [], None
    for b, plan in enumerate(plans):
        rng = np.random.default_rng(60 + b)
        st = {c: _fm_station(rng, B, tones.CTCSS[k], 10.0 ** (-(c % 5) / 4.0)) for c, k in plan.items()}
        x = squelch_model.sparse_band(N, ref.input_frequency, centres, B, st, seed=b)
        ref.load(x.astype(np.complex128))
        exp = squelch_model.levels(oracle, ref)
        if thr is None:
            thr = rc.tools.threshold_over_floor(exp, B, 10.0)
        assert squelch_model.margin_db(exp, thr) >= 3.0
        level_masks.append(squelch_model.open_mask(exp, thr))
        assert sorted(np.flatnonzero(level_masks[-1])) == sorted(plan)
        bufs.append(x)
    return dict(bufs=bufs, plans=plans, thr=thr, level_masks=level_masks)


def _tone_masks(audio, want, level_mask=None):
    """The model's tone squelch on the audio the device produced: float64 P and E, the score, the margin, the mask."""
    from radiocore.tools import tones
    P, E = tone_model.tone_bank(audio, np.array(tones.CTCSS) / AUDIO, AUDIO, tone_model.hann(AUDIO))
    score = tone_model.tone_score(P, E, want, level_mask)
    assert tone_model.margin(score, RATIO) >= 3.0, (tone_model.margin(score, RATIO), score)
    return tone_model.open_mask(score, RATIO)


def test_tuner_off_bank_and_tone_squelch(rc, fm_band):
    """set_tones(None) and a tuner that never heard of tones: the same audio.  With a bank: the same audio still, and
    tone_power() is rcfm_tone_bank_run on it.  With want and ratio: the model's mask; with a level squelch too: the AND."""
    import torch
    from radiocore.tools import tones
    x, plan = fm_band["bufs"][0], fm_band["plans"][0]
    plain, _ = _tuner(rc)
    plain.load(x)
    base = plain.run_all()
    t, _ = _tuner(rc)
    t.set_tones(None)
    t.load(x)
    assert np.array_equal(t.run_all().view(np.uint32), base.view(np.uint32))
    for call in (t.tone_power, t.open_mask):
        with pytest.raises(RuntimeError):
            call()
    bank = rc.ToneBank(tones.CTCSS)
    t.set_tones(bank)
    got = t.run_all()
    assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
    with pytest.raises(RuntimeError):
        t.open_mask()                                        # a bank alone is no squelch
    P, E = t.tone_power()
    assert P.shape == (C, 1, 39) and E.shape == (C, 1) and P.dtype == np.float32
    Pd, Ed = bank.run(torch.from_numpy(base).cuda(), step=1)
    assert np.array_equal(P, Pd.cpu().numpy()) and np.array_equal(E, Ed.cpu().numpy())
    best = tones.strongest(P, E, RATIO)[:, 0, 0]
    assert {c: int(best[c]) for c in plan} == plan           # every station's tone is named
    # tone squelch alone: empty channels demodulate to noise, which carries no tone
    want = [88.5] * C
    want[22] = None                                          # channel 22 needs no tone: open whatever it carries
    t.set_tones(bank, want=want, ratio=RATIO)
    got = t.run_all()
    want_idx = np.array([8] * C)
    want_idx[22] = -1
    tone_mask = _tone_masks(base, want_idx)
    assert sorted(np.flatnonzero(tone_mask)) == [1, 4, 15, 22]
    assert np.array_equal(t.open_mask(), tone_mask)
    _check_squelched(got, base, tone_mask, "tone squelch")
    assert np.array_equal(t.tone_power()[0], P)              # the powers do not depend on the squelch
    # level squelch and tone squelch together: the AND.  Channel 22 needs no tone but must pass the level; a level
    # threshold of +inf on channel 4 closes it although its tone is right
    thr = fm_band["thr"].copy()
    thr[4] = np.inf
    level_mask = fm_band["level_masks"][0].copy()
    level_mask[4] = False
    t.set_squelch(thr)
    got = t.run_all()
    both = _tone_masks(base, want_idx, level_mask)
    assert np.array_equal(both, tone_mask & level_mask) and sorted(np.flatnonzero(both)) == [1, 15, 22]
    assert np.array_equal(t.open_mask(), both)
    _check_squelched(got, base, both, "level and tone")
    assert np.array_equal(t.tone_power()[0], P)              # the bank runs before the level squelch
    # run_all_packed packs exactly the combined-open rows
    index, packed = t.run_all_packed(rc.PCM("float32"))
    assert index.tolist() == [1, 15, 22]
    assert np.array_equal(packed.view(np.uint32), base[[1, 15, 22]].view(np.uint32))
    # run_each: the same groups, the same masks
    each = t.run_each()
    assert np.array_equal(t.open_mask(), both)
    _check_squelched(np.stack(each), base, both, "run_each")
    assert np.array_equal(t.tone_power()[0], P)
    t.set_tones(None)
    t.set_squelch(None)
    assert np.array_equal(t.run_all().view(np.uint32), base.view(np.uint32))


def test_lanes_depth_two(rc, fm_band):
    """Lanes(depth=2) over two buffers: P, E, masks and audio equal the base tuner's, one buffer at a time."""
    from radiocore.tools import Lanes, tones
    bank = rc.ToneBank(tones.CTCSS)
    one, _ = _tuner(rc)
    one.set_squelch(fm_band["thr"])
    one.set_tones(bank, want=88.5, ratio=RATIO)
    expect = []
    for b, x in enumerate(fm_band["bufs"]):
        one.load(x)
        audio = one.run_all()
        expect.append((audio, one.open_mask(), one.tone_power()))
        assert sorted(np.flatnonzero(expect[-1][1])) == sorted(c for c, k in fm_band["plans"][b].items() if k == 8)
    base, _ = _tuner(rc)
    base.set_squelch(fm_band["thr"])
    base.set_tones(bank, want=88.5, ratio=RATIO)
    lanes = Lanes(base, depth=2)
    tickets = [lanes.submit(x) for x in fm_band["bufs"]]
    for (audio, mask, (P, E)), ticket in zip(expect, tickets):
        got, got_mask, (gP, gE) = lanes.result(ticket, open_mask=True, tones=True)
        assert np.array_equal(got.view(np.uint32), audio.view(np.uint32))
        assert np.array_equal(got_mask, mask)
        assert np.array_equal(gP, P) and np.array_equal(gE, E)
    base.set_tones(None)
    t0, t1 = lanes.submit(fm_band["bufs"][0]), lanes.submit(fm_band["bufs"][1])       # the second lane follows the setting
    assert lanes.result(t1, tones=True)[1] is None and lanes.result(t0, open_mask=True, tones=True)[2] is None


def test_wbfm_reads_the_left_channel_only(rc):
    """WBFM's audio is interleaved L, R: the Tuner's bank runs with step 2, offset 0 -- its powers are those of the left
    side alone, whatever the right side holds.  The Tuner's own run is never fed a spoiled right side (the demodulator
    writes both): the Tuner's P is compared with the model on the left side, which shows what the Tuner addressed, and with
    the bank run directly at step 2, offset 0 on a copy whose right side is NaN, which shows that this addressing reads
    nothing of the right side -- the same bits."""
    import torch
    from radiocore.tools import tones
    bw, A, chans = 60000, 12000, 3
    t, centres = _tuner(rc, "WBFM", bw, A, chans, n=600000)
    x = workloads.wideband(600000, t.input_frequency, centres, bw, gain=0.5)
    bank = rc.ToneBank(tones.SELCAL, frame=3000)
    t.set_tones(bank)
    t.load(x)
    audio = t.run_all()
    P, E = t.tone_power()
    assert audio.shape == (chans, A, 2) and P.shape == (chans, 4, 16) and E.shape == (chans, 4)
    left = np.ascontiguousarray(audio[:, :, 0])
    Pm, Em = tone_model.tone_bank(left, np.array(tones.SELCAL) / A, 3000, tone_model.hann(3000))
    top = tone_model.largest_power(left, 3000, tone_model.hann(3000))[..., None]
    assert np.max(np.abs(P - Pm) / top) <= 1e-5 and np.max(np.abs(E - Em) / Em) <= 1e-5
    spoiled = audio.copy()
    spoiled[:, :, 1] = np.nan
    Ps, Es = bank.run(torch.from_numpy(spoiled).cuda(), step=2, offset=0)
    assert np.array_equal(Ps.cpu().numpy(), P) and np.array_equal(Es.cpu().numpy(), E)


def test_pmr_tone_squelch_example():
    """examples/pmr_tone_squelch.py: its own assertions hold."""
    spec = importlib.util.spec_from_file_location("pmr_tone_squelch", os.path.join(ROOT, "examples", "pmr_tone_squelch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    results = mod.run(channels=16, rate=1_000_000, seconds=2)
    assert len(results) == 2 and all(len(on_air) == 5 and len(opened) == 2 for on_air, opened, _, _ in results)
    mod.check(results)
