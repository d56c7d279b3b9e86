"""Demodulators at odd, equal and up-sampling channel lengths: the case table, the stations, the float64 truth, deliberately
wrong models ("mutants") and the bound derived from them (no test functions; CPU only).

Decimate (decimate.py:21-50) follows scipy.signal.resample, whose Nyquist rule for real input has six branches, with
B = input_size, A = output_size and n = min(A, B):

    down_even   A < B, A even   bin n / 2 is doubled          down_odd   A < B, A odd   no Nyquist bin
    same_even   A = B, even     bin n / 2 is kept as it is    same_odd   A = B, odd
    up_even     A > B, B even   bin n / 2 is halved           up_odd     A > B, B odd

The library restates that rule per route (the engine's fused functors, the resampling kernels around rocFFT, the tiles'
refusals) and, for WBFM, the one-sided Hilbert mask for even and odd B and the same-size Hamming step as a three-tap
circular filter inside the pilot kernels, of which there are three forms by B % 4 and B % 8.  CASES crosses branches,
routes and pilot kernels; tests/test_length_cases.py holds the table to the library's plans (rcfm_fft_describe) and to
the model, tests/test_hip_lengths.py runs it on the device.

Stations -- station(kind, B, A, i): workloads.station_mpx under the modulation of workloads.station_iq (deviation 0.2 B
below B = 60 000, the default above; noise 0.01), plus, where n is even, a tone of `amp` at exactly n / 2 Hz in the
multiplex: the stations themselves put almost nothing into that bin, and a wrong factor there would pass unseen.  AM:
the carrier 1 + 0.5 m(t) with the same tone in the envelope.

Truth -- signal_edges.Truth (the oracle's chain on the float64 discriminator); for AM the specification of
include/rcfm.h (RCFM_AM) in float64 on the samples cast up.  ref32 is the same chain in float32, `reference` the
oracle itself (radiocore_oracle.FM / MFM / WBFM, am_model.expect).

Mutants -- the truth with ONE rule broken: the factor of bin n / 2 of the case's branch (1 instead of 2, 1 instead of
1 / 2, 2 where A = B; for WBFM with A = B the same in the same-size step alone), and for WBFM the circular wrap of the
same-size step dropped (sample 0 loses 0.23 d[B - 1]).  The odd branches have no bin n / 2 and no such mutant.

bound(kind, B, A) = min(conftest.TOL, smallest mutant distance of the case / 10): what the device is held to against
the truth.  It comes from the model alone; nothing a kernel returns enters it.  [measured ...] in the table is what
the MI355X returned (worst of three stations and two buffers, against the truth), next to that bound.
"""

import functools

import numpy as np

import am_model
import radiocore_oracle as oracle
import signal_edges as se
import workloads

TOL = 1e-4                      # conftest.TOL
STEP_CAP = 0.9                  # max |phase step| / pi of every FM station here
AMP = 0.15                      # the tone at n / 2 Hz, relative to the multiplex (AM: to the carrier)
BUFFERS = 2
ROWS = 3                        # stations per batched call
CLIP = se.CLIP

# (kind, B, A): (branch, route, pilot kernel) it is meant to reach.  route: "engine" where the FFT engine plans B and A,
# else "rocfft" (every transform of the demodulator).  pilot kernel (WBFM), by B: "h40" B % 8 == 0, "h40_ragged"
# B % 8 == 4 (a channel ends inside a thread's run of eight), "generic_even" B % 4 == 2, "generic_odd" B odd; and
# "h40_blocked" where B % 4 == 0 and the library reports the tile-blocked hand-over of m and p as effective
# (RCFM_OPT_PILOT_BLOCKED, read from the handle by the GPU test): k_pilot_stage_h40 then owns whole rows and has no
# ragged end, whatever B % 8 is.  48 000 = 200 x 240 is such a length; 62 500 = 250 x 250 is not (rows of 250 samples are
# no whole quads), and a planner that made it one would turn its label into "h40_blocked" and fail the table.
# Every comment: length_cases.bound as tests/test_length_cases.py prints it, then [measured: the batched call on an MI355X
# against the truth, worst of three stations and two buffers; the same against the oracle].
CASES = {
    ("FM", 23625, 7875): ("down_odd", "engine", None),                  # bound 1.00e-04 [measured 3.65e-07; vs the oracle 5.56e-07]
    ("FM", 23625, 8000): ("down_even", "engine", None),                 # bound 1.00e-04 [measured 4.68e-07; vs the oracle 6.11e-07]
    ("FM", 24000, 7875): ("down_odd", "engine", None),                  # bound 1.00e-04 [measured 3.75e-07; vs the oracle 5.16e-07]
    ("FM", 24000, 24000): ("same_even", "engine", None),                # bound 1.00e-04 [measured 5.69e-07; vs the oracle 8.43e-07]
    ("FM", 23625, 23625): ("same_odd", "engine", None),                 # bound 1.00e-04 [measured 4.99e-07; vs the oracle 8.12e-07]
    ("FM", 24000, 48000): ("up_even", "engine", None),                  # bound 1.00e-04 [measured 6.51e-07; vs the oracle 9.70e-07]
    ("FM", 23625, 48000): ("up_odd", "engine", None),                   # bound 1.00e-04 [measured 5.08e-07; vs the oracle 9.80e-07]
    ("FM", 24001, 8000): ("down_even", "rocfft", None),                 # bound 1.00e-04 [measured 5.00e-07; vs the oracle 6.88e-07]
    ("FM", 24002, 7999): ("down_odd", "rocfft", None),                  # bound 1.00e-04 [measured 5.59e-07; vs the oracle 7.74e-07]
    ("FM", 24002, 24002): ("same_even", "rocfft", None),                # bound 1.00e-04 [measured 8.81e-07; vs the oracle 1.01e-06]
    ("FM", 24001, 24001): ("same_odd", "rocfft", None),                 # bound 1.00e-04 [measured 7.29e-07; vs the oracle 9.80e-07]
    ("FM", 24002, 48000): ("up_even", "rocfft", None),                  # bound 1.00e-04 [measured 5.91e-07; vs the oracle 9.32e-07]
    ("FM", 24001, 48000): ("up_odd", "rocfft", None),                   # bound 1.00e-04 [measured 6.26e-07; vs the oracle 8.95e-07]
    ("MFM", 23625, 7875): ("down_odd", "engine", None),                 # bound 1.00e-04 [measured 4.56e-07; vs the oracle 5.72e-07]
    ("MFM", 23625, 8000): ("down_even", "engine", None),                # bound 1.00e-04 [measured 3.71e-07; vs the oracle 5.27e-07]
    ("MFM", 24000, 7875): ("down_odd", "engine", None),                 # bound 1.00e-04 [measured 5.00e-07; vs the oracle 5.71e-07]
    ("MFM", 24000, 24000): ("same_even", "engine", None),               # bound 1.00e-04 [measured 4.73e-07; vs the oracle 6.38e-07]
    ("MFM", 23625, 23625): ("same_odd", "engine", None),                # bound 1.00e-04 [measured 7.51e-07; vs the oracle 7.88e-07]
    ("MFM", 24000, 48000): ("up_even", "engine", None),                 # bound 1.00e-04 [measured 5.81e-07; vs the oracle 8.34e-07]
    ("MFM", 23625, 48000): ("up_odd", "engine", None),                  # bound 1.00e-04 [measured 4.56e-07; vs the oracle 5.93e-07]
    ("MFM", 24001, 8000): ("down_even", "rocfft", None),                # bound 1.00e-04 [measured 4.65e-07; vs the oracle 6.13e-07]
    ("MFM", 24002, 7999): ("down_odd", "rocfft", None),                 # bound 1.00e-04 [measured 5.58e-07; vs the oracle 7.64e-07]
    ("MFM", 24002, 24002): ("same_even", "rocfft", None),               # bound 1.00e-04 [measured 7.77e-07; vs the oracle 8.77e-07]
    ("MFM", 24001, 24001): ("same_odd", "rocfft", None),                # bound 1.00e-04 [measured 7.35e-07; vs the oracle 7.87e-07]
    ("MFM", 24002, 48000): ("up_even", "rocfft", None),                 # bound 1.00e-04 [measured 7.82e-07; vs the oracle 8.85e-07]
    ("MFM", 24001, 48000): ("up_odd", "rocfft", None),                  # bound 1.00e-04 [measured 8.64e-07; vs the oracle 9.86e-07]
    ("AM", 23625, 8000): ("down_even", "engine", None),                 # bound 1.00e-04 [measured 1.07e-06; vs the oracle 1.38e-06]
    ("AM", 24000, 24000): ("same_even", "engine", None),                # bound 1.00e-04 [measured 1.43e-06; vs the oracle 1.78e-06]
    ("AM", 23625, 23625): ("same_odd", "engine", None),                 # bound 1.00e-04 [measured 1.50e-06; vs the oracle 1.96e-06]
    ("AM", 24000, 48000): ("up_even", "engine", None),                  # bound 1.00e-04 [measured 1.53e-06; vs the oracle 2.17e-06]
    ("AM", 23625, 48000): ("up_odd", "engine", None),                   # bound 1.00e-04 [measured 1.60e-06; vs the oracle 2.12e-06]
    ("AM", 24001, 8000): ("down_even", "rocfft", None),                 # bound 1.00e-04 [measured 1.56e-06; vs the oracle 1.77e-06]
    ("AM", 24002, 24002): ("same_even", "rocfft", None),                # bound 1.00e-04 [measured 3.29e-06; vs the oracle 3.78e-06]
    ("AM", 24001, 24001): ("same_odd", "rocfft", None),                 # bound 1.00e-04 [measured 2.79e-06; vs the oracle 3.56e-06]
    ("AM", 24002, 48000): ("up_even", "rocfft", None),                  # bound 1.00e-04 [measured 2.40e-06; vs the oracle 2.48e-06]
    ("AM", 24001, 48000): ("up_odd", "rocfft", None),                   # bound 1.00e-04 [measured 2.45e-06; vs the oracle 2.66e-06]
    # the pilot band-pass design needs B > 38 100: these are the smallest practical WBFM lengths
    ("WBFM", 62500, 12500): ("down_even", "engine", "h40_ragged"),      # bound 1.00e-04 [measured 3.46e-06; vs the oracle 6.27e-06]
    ("WBFM", 60750, 12150): ("down_even", "engine", "generic_even"),    # bound 1.00e-04 [measured 1.34e-06; vs the oracle 1.77e-06]
    ("WBFM", 50625, 10125): ("down_odd", "engine", "generic_odd"),      # bound 2.56e-05 [measured 5.24e-07; vs the oracle 7.55e-07]
    ("WBFM", 50625, 12000): ("down_even", "engine", "generic_odd"),     # bound 1.00e-04 [measured 5.06e-07; vs the oracle 6.40e-07]
    ("WBFM", 48000, 48000): ("same_even", "engine", "h40_blocked"),     # bound 3.56e-05 [measured 7.00e-07; vs the oracle 1.10e-06]
    ("WBFM", 50625, 50625): ("same_odd", "engine", "generic_odd"),      # bound 2.60e-05 [measured 8.35e-07; vs the oracle 7.91e-07]
    ("WBFM", 48000, 60000): ("up_even", "engine", "h40_blocked"),       # bound 2.93e-05 [measured 8.05e-07; vs the oracle 1.20e-06]
    ("WBFM", 50625, 60000): ("up_odd", "engine", "generic_odd"),        # bound 2.53e-05 [measured 5.73e-07; vs the oracle 7.91e-07]
    ("WBFM", 60004, 12000): ("down_even", "rocfft", "h40_ragged"),      # bound 1.00e-04 [measured 6.45e-07; vs the oracle 8.58e-07]
    ("WBFM", 60002, 12001): ("down_odd", "rocfft", "generic_even"),     # bound 7.47e-05 [measured 8.78e-07; vs the oracle 1.13e-06]
    ("WBFM", 60001, 12000): ("down_even", "rocfft", "generic_odd"),     # bound 1.00e-04 [measured 7.74e-07; vs the oracle 9.60e-07]
    ("WBFM", 60002, 60002): ("same_even", "rocfft", "generic_even"),    # bound 4.57e-05 [measured 9.98e-07; vs the oracle 1.14e-06]
    ("WBFM", 60001, 60001): ("same_odd", "rocfft", "generic_odd"),      # bound 4.05e-05 [measured 1.03e-06; vs the oracle 1.10e-06]
    ("WBFM", 60002, 62500): ("up_even", "rocfft", "generic_even"),      # bound 4.41e-05 [measured 9.00e-07; vs the oracle 1.11e-06]
    ("WBFM", 60001, 62500): ("up_odd", "rocfft", "generic_odd"),        # bound 4.03e-05 [measured 7.92e-07; vs the oracle 1.04e-06]
}
# the tone's amplitude where the default leaves the mutants too close: WBFM up-sampling halves a bin whose two Hamming
# weights are 0.08 each; the room under STEP_CAP allows a stronger tone there
AMPS = {
    ("WBFM", 48000, 48000): 0.6,
    ("WBFM", 48000, 60000): 0.6,
    ("WBFM", 60002, 60002): 0.6,
    ("WBFM", 60002, 62500): 0.6,
}
BRANCHES = ("down_even", "down_odd", "same_even", "same_odd", "up_even", "up_odd")
# through the Tuner (C = 3, chunk = 2, two buffers, N = 10 int(1.25 B)): (kind, B, A); bound 1e-4 each, 2.56e-5 for 50 625 -> 10 125
# [measured, default route / fused_tiles=False, phase_link=False against the truth; the two against each other]
TUNER_CASES = [
    ("WBFM", 62500, 12500),    # phase link, h40 on phases with the ragged end [measured 8.21e-07 / 8.08e-06; 7.84e-06; phase_link=False alone 1.38e-06]
    ("WBFM", 60750, 12150),    # complex hand-over, generic pilot kernel: both settings launch the same kernels [measured 3.85e-07 / 3.85e-07; 0]
    ("WBFM", 50625, 10125),    # the same at odd B and A [measured 5.73e-07 / 5.73e-07; 0]
    ("MFM", 23625, 8000),      # phases of odd rows [measured 4.41e-07 / 4.43e-07; 3.48e-07]
    ("FM", 23625, 7875),       # [measured 4.38e-07 / 4.86e-07; 3.42e-07]
    ("AM", 24000, 48000),      # envelope link, up-sampling [measured 1.95e-06 / 1.82e-06; 1.86e-06]
]
# does the default route hand the demodulator phases (AM: envelopes) instead of complex samples?  The GPU test holds this
# to phase_capable() below and to the audio: with phase_link=False alone it changes in rounding where True, not a bit where False
TUNER_PHASE_LINK = {("WBFM", 62500, 12500): True, ("WBFM", 60750, 12150): False, ("WBFM", 50625, 10125): False,
                    ("MFM", 23625, 8000): True, ("FM", 23625, 7875): True, ("AM", 24000, 48000): True}


def branch(B, A):
    n = min(A, B)
    return ("down" if A < B else "same" if A == B else "up") + ("_even" if n % 2 == 0 else "_odd")


def pilot_kernel(kind, B, blocked=False):
    """The pilot kernel form by B; `blocked`: the library reports the tile-blocked hand-over of m and p as effective
    (RCFM_OPT_PILOT_BLOCKED) -- k_pilot_stage_h40 then owns whole rows and its ragged-end branch is never reached."""
    if kind != "WBFM":
        return None
    if B % 4:
        return "generic_odd" if B % 2 else "generic_even"
    return "h40_blocked" if blocked else "h40_ragged" if B % 8 else "h40"


def blocked_layout(plan):
    """kernels.hip, PilotBlocked::plan restated on the engine's plan of B (hip.FftPlan, or None): can m and p leave the
    pilot stage tile-blocked?  Necessary for an effective RCFM_OPT_PILOT_BLOCKED (the pilot chain must accept B too)."""
    if plan is None or plan.npass != 2:
        return False
    p0 = plan.passes[0]
    L, R, T = int(p0.L), int(p0.in_l), 2048
    if p0.load_along_l or p0.in_i != 1 or p0.n_o1 != 1 or p0.n_o2 != 1 or L * R != plan.n or p0.n_inner != R:
        return False                                         # fused_pilot_chain_geometry
    if R < 32 or R % 4 or R > T // 2 or L * R > 1 << 30:
        return False
    rpt = (T // R) & ~1
    return rpt >= 2 and rpt * R >= T - T // 8 and L * R >= 2 * T


def phase_capable(kind, B, plans_B):
    """demod.hip, rcfm_demod_s::phase_capable (and the tuner's: an engine for the band) restated: does rcfm_pipeline_run
    hand this demodulator phases (AM: envelopes) instead of complex samples when RCFM_OPT_PHASE_LINK is on?"""
    return bool(plans_B) and (kind != "WBFM" or B % 4 == 0)


# Where the resampling rule is applied.  "decim_tile": the decimating two-transform tile merges the bin itself (no
# audio_spectrum stage, for WBFM no ifft_A stage either); "resample_kernel": k_spectrum_r2c / k_spectrum_real_full /
# k_stereo_unpack as the audio_spectrum stage; "ifft_load": LoadStereoUnpack on the first pass of IFFT_A (WBFM on the
# engine has no audio_spectrum stage: the ifft_A stage marks it).  The GPU test reads the site from the stage profile and
# holds it to this: a case that moves between the tile and a separate resample is noticed.
# TILE_CASES: case -> (form, L, L2), the tile's kernel form ("run_time": k_fft_tile2_decim_rt, "instantiated":
# k_fft_tile2_decim) and its two transform lengths; tests/test_length_cases.py holds every row of CASES to the routing
# restated in tests/decim_cases.py (route()), whose own table takes the tile to every long length.
TILE_CASES = {("WBFM", 62500, 12500): ("run_time", 250, 50)}


def tile_of(kind, B, A):
    """(form, L, L2) where the decimating tile serves the case, else None."""
    return TILE_CASES.get((kind, B, A))


def resample_site(kind, B, A):
    if tile_of(kind, B, A) is not None:
        return "decim_tile"
    return "ifft_load" if kind == "WBFM" and CASES[(kind, B, A)][1] == "engine" else "resample_kernel"


def channels(kind):
    return 2 if kind == "WBFM" else 1


def amp_of(kind, B, A):
    return AMPS.get((kind, B, A), AMP) if min(A, B) % 2 == 0 else 0.0


# ---- stations ---------------------------------------------------------------------------------------------------------------

def station(kind, B, A, i, amp=None):
    """Station i of the case, complex64 [B] (module docstring)."""
    amp = amp_of(kind, B, A) if amp is None else amp
    t = np.arange(B, dtype=np.float64) / B
    n = min(A, B)
    tone = amp * np.cos(2 * np.pi * (n // 2) * t + 0.3) if amp and n % 2 == 0 else 0.0
    if kind == "AM":
        s = (1.0 + 0.5 * workloads.station_mpx(i, B, stereo=False) + tone).astype(np.complex128)
    else:
        deviation = 0.2 * B if B < 60000 else 75e3 * B / 240000.0
        mpx = workloads.station_mpx(i, B, stereo=(kind == "WBFM")) + tone
        s = np.exp(2j * np.pi * deviation * np.cumsum(mpx) / B)
    rng = np.random.default_rng(5000 + i)                    # workloads.station_iq's noise
    return (s + 0.01 * (rng.standard_normal(B) + 1j * rng.standard_normal(B))).astype(np.complex64)


def station_index(buf, row):
    """90 .. 95: well conditioned where the 38 kHz subcarrier aliases (signal_edges.clip_band)."""
    return 90 + buf + 2 * row


@functools.lru_cache(maxsize=None)
def signals(kind, B, A):
    """[buffer] -> complex64 [ROWS, B], read-only: row r of buffer b is station 90 + b + 2 r."""
    out = []
    for buf in range(BUFFERS):
        x = np.stack([station(kind, B, A, station_index(buf, r)) for r in range(ROWS)])
        x.setflags(write=False)
        out.append(x)
    return out


# ---- chains: truth, float32 restatement, the oracle, mutants ------------------------------------------------------------------

class Resample:
    """radiocore_oracle.Decimate written out on radiocore_oracle.resample_spectrum, with two rules that can be broken:
    nyq_gain multiplies bin n / 2 (n even) on top of what scipy's rule does to it, and wrap=False (A = B only) drops the
    two samples the same-size step fetches around the buffer's ends.  Defaults: Decimate itself."""

    def __init__(self, B, A, nyq_gain=1.0, wrap=True):
        self.B, self.A, self.nyq_gain, self.wrap = int(B), int(A), float(nyq_gain), bool(wrap)
        assert wrap or A == B
        self._win = oracle.shifted_window("hamm", self.B)

    def run(self, x):
        x = np.asarray(x)
        assert len(x) == self.B and np.isrealobj(x)
        Y = oracle.resample_spectrum(np.fft.rfft(x), self.A, self.B, True, self._win)
        n = min(self.A, self.B)
        if n % 2 == 0:
            Y[n // 2] *= self.nyq_gain
        y = np.fft.irfft(Y, self.A)
        y *= float(self.A) / float(self.B)
        if not self.wrap:
            # same size: y[i] = 0.54 x[i] + side (x[i - 1] + x[i + 1]), indices modulo B
            side = 0.23 * (np.cos(np.pi / self.B) if self.B % 2 else 1.0)
            y[0] -= side * x[-1]
            y[-1] -= side * x[0]
        return y


class AmTruth:
    """include/rcfm.h, RCFM_AM: e = |x|, v = Decimate(B, A)(e), audio = clip(v / mean(v) - 1); stateless."""

    def __init__(self, B, A, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self._decimate = oracle.Decimate(B, A)
        self.unclipped = self.mean = None

    def run(self, iq):
        e = np.abs(np.asarray(iq).astype(np.complex128)).astype(self.dtype)
        v = self._decimate.run(e)
        self.mean = np.mean(v)
        self.unclipped = (v / self.mean - 1)[:, None]
        return np.clip(self.unclipped, -CLIP, CLIP)


class _Reference:
    """The oracle's own demodulator (float32 unwrap and all), shaped [A, ch]."""

    def __init__(self, kind, B, A):
        self.kind, self.B, self.A = kind, B, A
        self._demod = getattr(oracle, kind)(B, A) if kind != "AM" else None

    def run(self, iq):
        if self.kind == "AM":
            return am_model.expect(oracle, iq, self.B, self.A)
        return np.asarray(self._demod.run(np.asarray(iq))).reshape(self.A, channels(self.kind))


def truth(kind, B, A, dtype=np.float64):
    """A fresh stateful chain: run(iq) -> [A, ch]; `unclipped` afterwards (None for FM)."""
    return AmTruth(B, A, dtype) if kind == "AM" else se.Truth(kind, B, A, dtype)


def ref32(kind, B, A):
    return truth(kind, B, A, np.float32)


def reference(kind, B, A):
    return _Reference(kind, B, A)


def mutants(kind, B, A):
    """{name: a fresh float64 chain with one rule broken}.  Deliberately wrong models."""
    out = {}

    def with_(**parts):
        c = truth(kind, B, A)
        for k, v in parts.items():
            setattr(c, k, v)
        return c

    br = branch(B, A)
    if br == "down_even":
        out["n/2 not doubled"] = with_(_decimate=Resample(B, A, nyq_gain=0.5))
    elif br == "up_even":
        out["n/2 not halved"] = with_(_decimate=Resample(B, A, nyq_gain=2.0))
    elif br == "same_even":
        out["n/2 doubled"] = with_(_decimate=Resample(B, A, nyq_gain=2.0))
        if kind == "WBFM":
            out["n/2 doubled in the same-size step"] = with_(_same=Resample(B, B, nyq_gain=2.0))
    if kind == "WBFM":
        out["same-size step without its wrap"] = with_(_same=Resample(B, B, wrap=False))
    return out


def distance(a, ref):
    """max|a - ref| / max|ref| (conftest.rel_err)."""
    return float(np.max(np.abs(np.asarray(a) - ref))) / float(np.max(np.abs(ref)))


@functools.lru_cache(maxsize=None)
def truths(kind, B, A):
    """[buffer][row] -> read-only float64 audio [A, ch] of signals(kind, B, A), the state carried across the buffers."""
    chains = [truth(kind, B, A) for _ in range(ROWS)]
    out = []
    for x in signals(kind, B, A):
        row = [chains[r].run(x[r]) for r in range(ROWS)]
        for a in row:
            a.setflags(write=False)
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def mutant_distances(kind, B, A):
    """{name: [distance of the mutant's audio from the truth, buffer after buffer, for every row in turn]} over all of
    signals(kind, B, A): the bound is applied to every row, so every row's stations enter it."""
    want = truths(kind, B, A)
    out = {}
    for r in range(ROWS):
        for name, chain in mutants(kind, B, A).items():     # fresh chains per row: each carries its row's state
            out.setdefault(name, []).extend(distance(chain.run(x[r]), want[buf][r])
                                            for buf, x in enumerate(signals(kind, B, A)))
    return out


def bound(kind, B, A, only=None):
    """min(TOL, smallest mutant distance / 10).  That every mutant lies 10 x bound away then holds by construction; what
    can fail is the other side: the float32 restatement and the oracle within bound / 10 (test_length_cases.py).
    `only`: the one mutant that counts (tests/decim_cases.py: "n/2 not doubled", the rule the decimating tile restates;
    the same-size step of WBFM is another kernel's), default all."""
    d = [v for name, per_signal in mutant_distances(kind, B, A).items() if only in (None, name) for v in per_signal]
    assert d or only is None, (kind, B, A, only)
    return min([TOL] + [v / 10.0 for v in d])
