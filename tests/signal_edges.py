"""Signal-content edges (no test functions): stations that drive the MFM / WBFM tails where workloads.station_iq never
goes, and the float64 evaluation they are compared with.

workloads.station_iq is a strong, clean, zero-mean station: its audio never reaches the clip of mfm.py:65 /
wbfm.py:100 and its discriminator mean is ~0.  The generators here keep its construction -- exp(j pi cumsum(m)), every
component of m with an integer-Hz period, so a one-second buffer of B samples is periodic -- and change the content:

    clipping_station   an asymmetric raised-cosine pulse train: after the mean is removed the pulses cross ONE clip bound
    dc_station         a carrier level * B / 2 Hz off the channel centre: the discriminator's mean is `level`

m is in discriminator units (phase step / pi), and every |m| stays at or below 0.85: the discriminator is then well
conditioned (tests/test_signal_edges.py pins that, on the samples the Tuner hands the demodulators).

Truth is the oracle's own chain (radiocore_oracle FM / MFM / WBFM) with `discriminator` replaced by
angle(x[t] conj x[t-1]) / pi in float64, everything downstream in float64 -- what
test_off_raster_stations_through_run_all patches into the oracle.  The reference's float32 unwrap (fm.py:62) is useless
at these carrier offsets, so this evaluation is the comparison target.  Truth(..., dtype=float32)
casts the float64 discriminator's output to float32 and runs the oracle's float32 chain from there: the reference's
arithmetic for the de-emphasis, np.mean and clip, which sets the scale for what a float32 mean can resolve.
"""

import numpy as np

import radiocore_oracle as oracle

CLIP = 0.999
STEP_BOUND = 0.85        # max |phase step| / pi of every generator
PULSES = 50              # pulses per buffer
DUTY = 0.10


def _periodic(m):
    """m nudged by a constant (< 2 / len(m)) so that pi * sum(m) is a multiple of 2 pi: exp(j pi cumsum(m)) then closes on
    itself at the buffer's end."""
    s = float(np.sum(m))
    return m + (2.0 * np.round(s / 2.0) - s) / len(m)


def _iq(m):
    return np.exp(1j * np.pi * np.cumsum(_periodic(m)))


def _tones(rng, t, freqs, amp):
    acc = np.zeros(len(t))
    for f in freqs:
        acc += amp * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return acc


def _stereo_parts(rng, t, k, amp):
    """(pilot, L - R on the 38 kHz subcarrier) of workloads.station_mpx's multiplex, the difference signal at peak `amp`."""
    diff = _tones(rng, t, (440 + 29 * k, 1500 + 7 * k), 0.5 * amp)
    return np.sin(2 * np.pi * 19000 * t), diff * np.sin(2 * np.pi * 38000 * t)


def clipping_station(B, i, sign=1, stereo=False):
    """Station i, complex128 [B]: PULSES raised-cosine pulses of DUTY / PULSES seconds on a base level, base -0.6 and peak
    +0.8 (stereo: +0.7, leaving room for a 0.08 pilot and a 0.05 L - R subcarrier) times `sign`, plus a 1 kHz tone of 0.01.
    The mean is about -0.53 sign: once it is removed the pulse tops stand at about 1.3 sign and ~3 % of the audio clips
    at the bound of that sign; the base, at -0.07 sign, stays far from the other bound.  The pulse centres are drawn per
    station within +-10 % of their slot, so no two pulses meet the audio's sampling grid alike: the number of samples
    that land within rounding of the bound is then a matter of measure, not of a pattern repeating 50 times."""
    rng = np.random.default_rng(3000 + i)
    t = np.arange(B, dtype=np.float64) / B
    base, peak = -0.6, (0.7 if stereo else 0.8)
    width = DUTY / PULSES
    centres = (np.arange(PULSES) + 0.5 + rng.uniform(-0.1, 0.1, PULSES)) / PULSES
    m = np.full(B, base)
    for c in centres:
        u = (t - c) / width
        inside = np.abs(u) < 0.5
        m[inside] += (peak - base) * 0.5 * (1.0 + np.cos(2 * np.pi * u[inside]))
    m += 0.01 * np.sin(2 * np.pi * 1000 * t + rng.uniform(0, 2 * np.pi))
    m *= float(sign)
    if stereo:
        pilot, sub = _stereo_parts(rng, t, i % 89, 0.05)
        m += 0.08 * pilot + sub
    return _iq(m)


def dc_station(B, i, level, stereo=False):
    """Station i, complex128 [B]: a carrier level * B / 2 Hz off the channel centre (the discriminator then averages
    `level`) under three symmetric tones of 0.12 between 300 Hz and 1.2 kHz, below every audio rate's Nyquist frequency
    and with drawn phases -- present in the last 50 audio samples as anywhere else.  Stereo: tones of 0.06, a 0.1 pilot
    and a 0.12 L - R subcarrier.  |m| <= |level| + 0.4 either way, and the audio (mean removed) peaks below 0.45."""
    offset = level * B / 2.0
    assert offset == int(offset), "level * B / 2 must be an integer number of Hz"
    rng = np.random.default_rng(4000 + i)
    t = np.arange(B, dtype=np.float64) / B
    k = i % 89
    m = np.full(B, float(level)) + _tones(rng, t, (300 + 7 * k, 700 + 3 * k, 1100 + k), 0.06 if stereo else 0.12)
    if stereo:
        pilot, sub = _stereo_parts(rng, t, k, 0.12)
        m += 0.1 * pilot + sub
    return _iq(m)


def wideband_from(stations, N, f_in, centres, B, gain=0.3, noise=0.0, seed=7):
    """complex64 [N] buffer with stations[i] (complex [B]) on centres[i], in the manner of workloads.wideband: each B-point
    spectrum is added at bin offset int(f_c - f_in), scaled so that the station's time-domain amplitude is `gain` (a
    scalar or one per station)."""
    gains = np.broadcast_to(np.asarray(gain, np.float64), (len(stations),))
    Xw = np.zeros(N, np.complex128)
    kk = np.fft.fftfreq(B, 1.0 / B).astype(np.int64)
    for fc, s, g in zip(centres, stations, gains):
        np.add.at(Xw, (kk + int(fc - f_in)) % N, np.fft.fft(s) * (g * N / B))
    x = np.fft.ifft(Xw)
    if noise:
        rng = np.random.default_rng(seed)
        x += noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return x.astype(np.complex64)


def steps(iq):
    """angle(x[t] conj x[t-1]) / pi in float64, d[0] = 0 (fm.py:64's pad)."""
    z = np.asarray(iq).astype(np.complex128)
    d = np.zeros(len(z))
    d[1:] = np.angle(z[1:] * np.conj(z[:-1])) / np.pi
    return d


class Truth:
    """truth(kind, B, A): stateful, like the oracle's demodulators -- consecutive buffers carry the de-emphasis state.
    run(iq) -> [A, ch]; afterwards `unclipped` holds the audio before np.clip and `mean` what was subtracted."""

    def __init__(self, kind, B, A, dtype=np.float64):
        self.kind, self.B, self.A, self.dtype = kind, int(B), int(A), np.dtype(dtype)
        self.ch = 2 if kind == "WBFM" else 1
        if kind == "WBFM":                                    # wbfm.py:44-57
            self._same = oracle.Decimate(B, B)
            self._pilot = oracle.Bandpass(B, 19e3 - 50, 19e3 + 50, num_taps=41)
            self._pll = oracle.PLL()
        self._decimate = oracle.Decimate(B, A)
        self._deemph = [oracle.Deemphasis(A, 75e-6) for _ in range(self.ch)] if kind != "FM" else []
        self.unclipped = self.mean = None

    def run(self, iq):
        d = steps(iq).astype(self.dtype)
        if self.kind == "FM":                                 # fm.py:60-67
            self.unclipped, self.mean = None, 0.0
            return self._decimate.run(d)[:, None]
        if self.kind == "MFM":                                # mfm.py:62-66
            a = self._deemph[0].run(self._decimate.run(d))
            self.mean = np.mean(a)
            a = a - self.mean
            self.unclipped = a[:, None]
            return np.clip(a, -CLIP, CLIP)[:, None]
        m = self._same.run(d)                                 # wbfm.py:66-100
        self._pll.step(self._pilot.run(m))
        lmr = (self._pll.image(2) * m) * 1.0175
        l = self._deemph[0].run(self._decimate.run(m + lmr))
        r = self._deemph[1].run(self._decimate.run(m - lmr))
        lr = np.dstack((l, r))
        self.mean = np.mean(lr)
        lr = lr - self.mean
        self.unclipped = lr[0]
        return np.clip(lr, -CLIP, CLIP)[0]


def truth(kind, B, A):
    return Truth(kind, B, A)


def ref32(kind, B, A):
    return Truth(kind, B, A, dtype=np.float32)


# ---- the bands the tests run: one place, so that test_signal_edges.py pins exactly what test_hip_signal_edges.py feeds ----

# (kind, N, B, A, C): the geometries of the clip and DC tests.  Channels on a raster of 7 B / 6 (whole Hz) around the
# band's centre: no overlap.  The Tuner's Hann weight tilts the outer 240 kHz channels (0.96 -> 0.75 across one); the step
# bound is therefore checked on the samples the oracle's Tuner returns, not on the stations.
FUSED = [("MFM", 1_200_000, 60000, 12000, 5), ("WBFM", 1_200_000, 60000, 12000, 5),
         ("MFM", 2_400_000, 240000, 48000, 3), ("WBFM", 2_400_000, 240000, 48000, 3)]
GENERIC = [("MFM", 1_200_000, 60000, 12150, 3), ("MFM", 1_200_000, 60000, 12006, 3), ("WBFM", 1_200_000, 60000, 12006, 3)]
LDS_ROWS = [("MFM", 1_000_000, 12500, 8000, 9), ("MFM", 1_000_000, 12500, 5000, 9), ("MFM", 1_000_000, 10000, 5000, 9),
            ("MFM", 1_000_000, 12000, 6000, 9), ("MFM", 1_000_000, 8000, 4000, 9)]
GEOMETRIES = FUSED + GENERIC + LDS_ROWS
BUFFERS = 3
DC_LEVELS = (0.4, -0.4)


def centres_of(B, C):
    import workloads
    return workloads.channel_grid(C, int(B * 7 / 6))


def clip_band(kind, N, B, C, f_in, buf):
    """Buffer `buf` of the clip test's band: channels alternate +, - clipping stations, the middle channel carries an
    ordinary workloads station; station indices move with the buffer.  Returns (x, signs) with signs[i] in (+1, -1, 0)."""
    import workloads
    stereo = kind == "WBFM"
    signs = [0 if i == C // 2 else (1 if (i - (i > C // 2)) % 2 == 0 else -1) for i in range(C)]
    # (stations 90 .. 92: at B = 60 000 the 38 kHz subcarrier aliases, and some stereo stations of workloads.station_iq
    #  are then ill conditioned by themselves -- tests/golden_cases.py has one; these are not, test_signal_edges.py checks)
    st = [workloads.station_iq(90 + buf, B, stereo=stereo, deviation=None if B >= 60000 else 0.2 * B) if s == 0
          else clipping_station(B, i + 11 * buf, s, stereo) for i, s in enumerate(signs)]
    return wideband_from(st, N, f_in, centres_of(B, C), B), signs


def dc_band(kind, N, B, C, f_in, buf):
    """Buffer `buf` of the DC test's band: channel i carries dc_station at level DC_LEVELS[i % 2] in every buffer (a
    channel that changed its level would start the next buffer with a 0.8 step, which clips), the station index -- tones
    and phases -- moves with the buffer.  Returns (x, levels)."""
    stereo = kind == "WBFM"
    levels = [DC_LEVELS[i % 2] for i in range(C)]
    st = [dc_station(B, i + 13 * buf, lv, stereo) for i, lv in enumerate(levels)]
    return wideband_from(st, N, f_in, centres_of(B, C), B), levels


def oracle_tuner(B, C, N, demodulators=None):
    """radiocore_oracle.Tuner over centres_of(B, C), N samples per buffer."""
    ref = oracle.Tuner()
    for i, f in enumerate(centres_of(B, C)):
        ref.add_channel(f, B, demodulators[i] if demodulators else None)
    ref.request_bandwidth(float(N))
    return ref


def evaluate(what, geometry, with_ref32=False, perturb=0.0):
    """The band `what` ("clip" / "dc") of `geometry` over BUFFERS consecutive buffers through the oracle's Tuner
    (run_pruned: the brick-wall truncation is shared with the device) and the float64 truth of every channel.  Returns one
    dict per buffer: x (the wideband buffer), tags (clip signs / DC levels), iq, truth, unclipped, mean -- lists over the
    channels -- plus ref32 (the float32 tail's audio) when with_ref32, and cond when perturb: the truth's largest change
    relative to its peak when every channel sample of every buffer so far is moved by `perturb` of its magnitude in a
    drawn direction."""
    kind, N, B, A, C = geometry
    ref = oracle_tuner(B, C, N)
    t64 = [Truth(kind, B, A) for _ in range(C)]
    t32 = [Truth(kind, B, A, np.float32) for _ in range(C)] if with_ref32 else None
    twin = [Truth(kind, B, A) for _ in range(C)] if perturb else None
    rng = np.random.default_rng(17)
    out = []
    for buf in range(BUFFERS):
        x, tags = (clip_band if what == "clip" else dc_band)(kind, N, B, C, ref.input_frequency, buf)
        ref.load(x)
        rec = {"x": x, "tags": tags, "iq": [], "truth": [], "unclipped": [], "mean": [], "ref32": [], "cond": []}
        for i in range(C):
            iq = ref.run_pruned(i)
            rec["iq"].append(iq)
            rec["truth"].append(t64[i].run(iq))
            rec["unclipped"].append(t64[i].unclipped)
            rec["mean"].append(float(t64[i].mean))
            if with_ref32:
                rec["ref32"].append(t32[i].run(iq))
            if perturb:
                moved = iq * (1.0 + perturb * np.exp(2j * np.pi * rng.uniform(size=len(iq))))
                delta = np.max(np.abs(twin[i].run(moved) - rec["truth"][-1]))
                rec["cond"].append(float(delta / np.max(np.abs(rec["truth"][-1]))))
        out.append(rec)
    return out
