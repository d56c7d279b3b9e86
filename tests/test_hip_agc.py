"""GPU: the stateful AGC (include/rcfm.h: rcfm_agc, rcfm_demod_set_agc) against tests/agc_model.py.

The primitive in both modes against the float64 definition on the same float32 input -- audio relative to the row's peak,
state relative to itself, each within min(max(4 x the float32 yardstick's own error, 1e-6), 1e-4) --, bit-identity (run
to run, streams, row sub-ranges, in place, chunks), AM / USB / LSB with `agc` against am_model / ssb_model + agc_model at
1e-4 of the peak, the pause the feature is for, and the Tuner: mixed run_each, run_all, state shared with the channels'
demodulator objects, squelch, shard, Lanes.

Worst figures measured on MI355X are recorded in DESIGN.md section 3.13.
"""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import agc_model as m
import am_model
import ssb_model
import workloads
from conftest import ROOT, TOL, have_gpu, rel_err
from test_hip_am import _Profile

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

MODES = [m.PEAK, m.CARRIER]
IDS = ["PEAK", "CARRIER"]


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def oracle():
    import radiocore_oracle
    return radiocore_oracle


@pytest.fixture(scope="module")
def hip(rc):
    from radiocore._internal import hip
    return hip


def _agc(hip, v, mode, params, state, out=None):
    """rcfm_agc on device tensors v [C, n] and state [C] (updated); -> audio (a new tensor unless `out` is given)."""
    t = hip.torch()
    C, n = v.shape
    out = t.empty_like(v) if out is None else out
    decay, level, floor = params
    hip.check(hip.lib().rcfm_agc(C, n, mode, float(decay), float(level), float(floor), hip.ptr(state), hip.ptr(v),
                                 hip.ptr(out), hip.stream()))
    return out


def _dev(hip, a):
    return hip.to_device(np.array(a, dtype=np.float32, order="C"))          # a copy: the model's arrays are read-only


# ---- the primitive -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("n", m.SIZES)
@pytest.mark.parametrize("case", m.CASES)
def test_primitive_against_float64(hip, case, n, mode):
    """Two calls with the state carried from -1 (the start rule), three rows over three decades of amplitude."""
    ref = m.reference(case, mode, n)
    v = ref["v"]
    state = _dev(hip, np.full(3, -1.0))
    for call in range(v.shape[0]):
        got = hip.to_host(_agc(hip, _dev(hip, v[call]), mode, ref["params"], state))
        st = hip.to_host(state)
        for r in range(3):
            if np.isnan(ref["audio"][call, r]).any():
                continue                                     # the row with the NaN may be spoiled; its neighbours may not
            assert not np.isnan(got[r]).any(), (call, r)
            if case == "zeros":
                assert not got[r].any() and st[r] == 0.0
                continue
            ea = m.audio_error(got[r], ref["audio"][call, r])
            es = m.state_error(st[r], ref["state"][call, r])
            ba, bs = m.bound(ref["yard_audio"][call, r]), m.bound(ref["yard_state"][call, r])
            print("%s %s n=%d call %d row %d: audio %.3g (bound %.3g)  state %.3g (bound %.3g)"
                  % (case, IDS[mode], n, call, r, ea, ba, es, bs))
            assert ea <= ba and es <= bs, (call, r, ea, ba, es, bs)


@pytest.mark.parametrize("mode", MODES, ids=IDS)
def test_one_row_of_2000_against_two_calls_of_1000(hip, mode):
    v = np.stack([m.voice(2000, 70 + r, mode) * a for r, a in enumerate(m.AMPLITUDES)])
    params = (700.0, 0.25 if mode == m.PEAK else 1.0, 1e-5)
    s0 = np.array(m.AMPLITUDES) * 0.4            # a history: without one CARRIER starts from the mean of the CALL's row
    one_state, two_state = _dev(hip, s0), _dev(hip, s0)
    one = hip.to_host(_agc(hip, _dev(hip, v), mode, params, one_state))
    two = np.concatenate([hip.to_host(_agc(hip, _dev(hip, v[:, :1000]), mode, params, two_state)),
                          hip.to_host(_agc(hip, _dev(hip, v[:, 1000:]), mode, params, two_state))], axis=1)
    for r in range(3):
        want, s_want = m.truth(v[r], mode, *params, s0[r])
        yard, s_yard = m.yardstick(v[r], mode, *params, s0[r])
        ba, bs = m.bound(m.audio_error(yard, want)), m.bound(m.state_error(s_yard, s_want))
        for name, got, st in (("one call", one, one_state), ("two calls", two, two_state)):
            ea, es = m.audio_error(got[r], want), m.state_error(hip.to_host(st)[r], s_want)
            print(IDS[mode], name, "row", r, "audio %.3g (bound %.3g) state %.3g (bound %.3g)" % (ea, ba, es, bs))
            assert ea <= ba and es <= bs
        assert m.audio_error(one[r], two[r]) <= ba


@pytest.mark.parametrize("mode", MODES, ids=IDS)
@pytest.mark.parametrize("n", [1000, 1001, 20000])
def test_primitive_bit_identity(hip, mode, n):
    """Run to run, on a second stream, rows 1 - 2 alone against rows 1 - 2 of three, in place, and from an address that is
    not 16-byte aligned (scalar loads instead of 16-byte ones)."""
    t = hip.torch()
    v = np.stack([m.voice(n, 80 + r, mode) * a for r, a in enumerate(m.AMPLITUDES)])
    params = (m.decay_for(n), 0.25 if mode == m.PEAK else 1.0, 1e-5)
    s0 = np.array([-1.0, 0.02, 0.0005])

    def run(rows=slice(0, 3), in_place=False, shift=0):
        vv = v[rows]
        state = _dev(hip, s0[rows])
        if shift:
            pad = t.zeros(vv.size + shift, dtype=t.float32, device="cuda")
            src = pad[shift:].view(vv.shape)
            src.copy_(_dev(hip, vv))
        else:
            src = _dev(hip, vv)
        out = _agc(hip, src, mode, params, state, out=src if in_place else None)
        return hip.to_host(out), hip.to_host(state)

    a0, s_0 = run()
    a1, s_1 = run()
    assert np.array_equal(a0, a1) and np.array_equal(s_0, s_1)
    with t.cuda.stream(t.cuda.Stream()):
        a2, s_2 = run()
        t.cuda.current_stream().synchronize()
    assert np.array_equal(a0, a2) and np.array_equal(s_0, s_2)
    a3, s_3 = run(rows=slice(1, 3))
    assert np.array_equal(a0[1:], a3) and np.array_equal(s_0[1:], s_3)
    a4, s_4 = run(in_place=True)
    assert np.array_equal(a0, a4) and np.array_equal(s_0, s_4)
    a5, s_5 = run(shift=1)
    assert np.array_equal(a0, a5) and np.array_equal(s_0, s_5)


# ---- AM / USB / LSB with agc -------------------------------------------------------------------------------------------

def _chain(rc, oracle, kind, B, A, **kw):
    iqs = [m.chain_iq(kind, B, buf) for buf in range(3)]
    vs = [m.chain_signal(oracle, kind, x, B, A) for x in iqs]
    floor = m.chain_floor(vs)
    want, s_want = m.follow(vs, m.chain_mode(kind), m.chain_settings(kind, A, floor))
    d = getattr(rc, kind)(B, A, agc=rc.AGC(m.CHAIN_DECAY, floor=floor), **kw)
    return d, iqs, want, s_want


@pytest.mark.parametrize("kind", ["AM", "USB", "LSB"])
@pytest.mark.parametrize("B,A", m.CHAIN_SIZES)
def test_classes_against_the_model(rc, oracle, kind, B, A):
    """Three consecutive buffers whose station level steps x10 and back; 3001 is prime: rocFFT, no DC bin."""
    d, iqs, want, s_want = _chain(rc, oracle, kind, B, A)
    assert d.agc_state().tolist() == [-1.0]
    first = None
    for buf in range(3):
        with _Profile() as ran:
            got = d.run(iqs[buf])
        first = got if first is None else first
        assert got.shape == (A, 1) and got.dtype == np.float32
        e = rel_err(got[:, 0], want[buf])
        print(kind, B, A, "buffer", buf, "rel err %.3g" % e)
        assert e <= TOL
        assert ran["am_tail" if kind == "AM" else "ssb_tail"] == 1, ran       # the AGC tail, timed as the stage it replaces
    assert m.state_error(d.agc_state()[0], s_want) <= TOL
    d.reset()
    assert d.agc_state().tolist() == [-1.0]
    assert np.array_equal(d.run(iqs[0]), first)


def _stations(kind, B, buf):
    mk = am_model.station if kind == "AM" else ssb_model.station
    return np.stack([mk(i, B, seed=60 + buf, level=0.3) for i in range(5)]).astype(np.complex64)


@pytest.mark.parametrize("kind", ["USB", "LSB"])
def test_chunk_1_against_the_default_chunk(rc, kind):
    """A batch of five channels with chunk = 1 against the default chunk, bit for bit, audio and state.  The geometry is
    one whose chain in front of the tail is itself independent of the chunk (3001 -> 1000, USB / LSB, every transform
    through rocFFT; the test checks that on the handles without agc first).  Elsewhere it is not, with or without agc: on
    the engine's geometries two channels share one complex transform, so a channel's rounding depends on its partner and
    hence on the chunk, and AM's real transform through rocFFT differs between a batch of one and a batch of five
    (measured: AM 3001 -> 1000 without agc, chunk = 1 against the default, is not bit-identical).  The next test covers
    those."""
    B, A = 3001, 1000
    xs = [_stations(kind, B, buf) for buf in range(2)]
    cls = getattr(rc, kind)
    assert np.array_equal(cls(B, A, batch=5).run(xs[0]), cls(B, A, batch=5, chunk=1).run(xs[0]))
    agc = rc.AGC(0.3, floor=0.03)
    whole, ones = cls(B, A, batch=5, agc=agc), cls(B, A, batch=5, chunk=1, agc=agc)
    for buf in range(2):
        assert np.array_equal(whole.run(xs[buf]), ones.run(xs[buf])), buf
    assert np.array_equal(whole.agc_state(), ones.agc_state()) and (whole.agc_state() > 0).all()


@pytest.mark.parametrize("kind", ["AM", "USB"])
def test_chunks_address_their_own_state(rc, kind):
    """On the engine (25 000 -> 8000): a batch of five with chunk = 1 is bit-identical to five one-channel demodulators,
    audio and state -- every chunk reads and writes its own channels' slots.  Against the default chunk the audio agrees
    within the chain's float32 rounding only: there channels 0 - 3 travel in pairs through one complex transform."""
    B, A = 25000, 8000
    xs = [_stations(kind, B, buf) for buf in range(2)]
    agc = rc.AGC(0.3, floor=0.03)
    cls = getattr(rc, kind)
    whole, ones = cls(B, A, batch=5, agc=agc), cls(B, A, batch=5, chunk=1, agc=agc)
    single = [cls(B, A, agc=agc) for _ in range(5)]
    for buf in range(2):
        a, b = whole.run(xs[buf]), ones.run(xs[buf])
        for i in range(5):
            assert np.array_equal(b[i], single[i].run(xs[buf][i])), (buf, i)
        e = max(rel_err(a[i], b[i]) for i in range(5))
        print(kind, "buffer", buf, "default chunk against chunk = 1: %.3g" % e)
        assert e <= TOL
    assert np.array_equal(ones.agc_state(), np.concatenate([s.agc_state() for s in single]))


def test_state_entry_points_and_switching_off(rc, hip):
    """rcfm_demod_set_agc_state puts a saved state back (the next buffer repeats bit for bit); decay_samples = 0 switches
    the AGC off again (the audio is that of a handle that never had one, the state entry points answer RCFM_ERR_STATE);
    other kinds are refused."""
    B, A = 3001, 1000
    lib = hip.lib()
    assert lib.rcfm_demod_set_agc(rc.FM(B, A)._handle.value, 2400.0, 0.25, 0.0) == -4
    d = rc.USB(B, A, batch=3, agc=rc.AGC(0.3, floor=0.03))
    xs = [_stations("USB", B, buf)[:3] for buf in range(2)]
    d.run(xs[0])
    saved = d.agc_state()
    a1 = d.run(xs[1])
    assert not np.array_equal(d.agc_state(), saved)
    buf = (ctypes.c_float * 3)(*saved)
    hip.check(lib.rcfm_demod_set_agc_state(d._handle.value, buf, hip.stream()))
    assert np.array_equal(d.agc_state(), saved)
    assert np.array_equal(d.run(xs[1]), a1)
    hip.check(lib.rcfm_demod_set_agc(d._handle.value, 0.0, 0.0, 0.0))
    assert np.array_equal(d.run(xs[1]), rc.USB(B, A, batch=3).run(xs[1]))
    assert lib.rcfm_demod_get_agc_state(d._handle.value, buf, hip.stream()) == -5


def test_graph_option_does_not_capture_an_agc_handle(rc, hip):
    """RCFM_OPT_GRAPH on a handle with AGC: the chain is launched, never captured, and the audio is what it is without."""
    B, A = 25000, 8000
    x = ssb_model.station(1, B, seed=5, level=0.3).astype(np.complex64)
    plain, graphed = (rc.USB(B, A, cuda=True, agc=rc.AGC(0.3, floor=0.03)) for _ in range(2))
    hip.check(hip.lib().rcfm_demod_set_option(graphed._handle.value, hip.RCFM_OPT_GRAPH, 1))
    xd = hip.to_device(x)
    for _ in range(4):                               # the same pointers four times: a handle without AGC captures on the second
        a = plain.run(xd)
        b = graphed.run(xd)
        assert np.array_equal(a, b)
    value = ctypes.c_int(-1)
    hip.check(hip.lib().rcfm_demod_get_option(graphed._handle.value, hip.RCFM_OPT_GRAPH, ctypes.byref(value)))
    assert value.value == 1                          # on, and no captured chain


# ---- the point of the feature ------------------------------------------------------------------------------------------

def test_a_pause_no_longer_raises_the_gain(rc):
    """A constant tone with half a second of silence in buffer 2.  With agc the tone's projected amplitude is within 1 % of
    `level` in all three buffers; with the per-buffer RMS, buffer 2 comes out more than 2 dB off its neighbours."""
    B, A, f, level = 12500, 8000, 1037, 0.25
    t = np.arange(B) / B
    gate = np.clip((0.5 - t) / 0.02, 0.0, 1.0)
    gate = 0.5 - 0.5 * np.cos(np.pi * gate)                 # on for 0.48 s, a 20 ms raised-cosine fall, then silence
    tone = 0.2 * np.exp(2j * np.pi * f * t)
    bufs = [tone, tone * gate, tone]
    k = np.arange(int(0.05 * A), int(0.40 * A))             # where the tone is on in every buffer

    def amplitude(audio):
        return 2.0 * abs(np.mean(audio[k, 0].astype(np.float64) * np.exp(-2j * np.pi * f * k / A)))
    with_agc, without = rc.USB(B, A, agc=rc.AGC(1.0, level=level)), rc.USB(B, A)
    amp_agc = [amplitude(with_agc.run(x.astype(np.complex64))) for x in bufs]
    amp_rms = [amplitude(without.run(x.astype(np.complex64))) for x in bufs]
    print("with agc", amp_agc, "per-buffer RMS", amp_rms)
    assert all(abs(a - level) <= 0.01 * level for a in amp_agc), amp_agc
    db = [20 * np.log10(amp_rms[1] / amp_rms[i]) for i in (0, 2)]
    assert all(abs(d) > 2.0 for d in db), db


# ---- the Tuner ---------------------------------------------------------------------------------------------------------

N, B, A, C = 600_000, 25000, 8000, 24
KINDS = (["AM"] * 4 + ["USB"] * 4 + ["LSB"] * 4) * 2
WITH_AGC = [True] * 12 + [False] * 12           # the first block of each class with agc, the second without
FLOOR = {"AM": 0.06, "USB": 0.17, "LSB": 0.17}   # >= 0.1 of the rows' peaks (envelopes up to 0.55, sidebands up to 1.65; the band fixture checks it)


@pytest.fixture(scope="module")
def band(oracle):
    """Three buffers of a seeded band, the oracle's channel samples, and the expected audio per buffer and channel for
    a Tuner whose channels i with agc[i] carry AGC(0.3, floor=FLOOR[kind]) -- computed once, never modified."""
    centres = workloads.channel_grid(C, B)
    ref = oracle.Tuner()
    for f in centres:
        ref.add_channel(f, B, None)
    ref.request_bandwidth(float(N))
    xs, vs = [], []
    for buf in range(4):
        st = [(am_model.station if k == "AM" else ssb_model.station)(i, B, seed=70 + buf, level=0.3)
              for i, k in enumerate(KINDS)]
        x = am_model.wideband(N, ref.input_frequency, centres, B, st, seed=70 + buf)
        ref.load(x)
        xs.append(x)
        vs.append([m.chain_signal(oracle, KINDS[i], ref.run_pruned(i), B, A) for i in range(C)])
    for i, k in enumerate(KINDS):
        assert FLOOR[k] >= 0.1 * max(np.max(np.abs(vs[b][i])) for b in range(4)), (i, k)
    return {"centres": centres, "x": xs, "v": vs, "f_in": ref.input_frequency}


def _settings(kind):
    return m.chain_settings(kind, A, FLOOR[kind])


def _expected(band, oracle, i, nbuf, start=0):
    """[audio] of channel i over buffers start .. start + nbuf - 1 with the AGC state carried from -1, and the last state."""
    return m.follow([band["v"][b][i] for b in range(start, start + nbuf)], m.chain_mode(KINDS[i]), _settings(KINDS[i]))


def _tuner(rc, band, agc=WITH_AGC, **options):
    t = rc.Tuner()
    for i, f in enumerate(band["centres"]):
        kw = {"agc": rc.AGC(m.CHAIN_DECAY, floor=FLOOR[KINDS[i]])} if agc[i] else {}
        t.add_channel(f, B, getattr(rc, KINDS[i])(B, A, **kw))
    t.request_bandwidth(float(N))
    assert t.input_frequency == band["f_in"]
    if options:
        t.set_kernel_options(**options)
    return t


@pytest.mark.parametrize("options", [{}, {"ssb_direct": False, "phase_link": False}], ids=["default", "general"])
def test_tuner_run_each_mixed(rc, oracle, band, options):
    """AM, USB and LSB, with and without agc, over three buffers: the AGC channels follow the model, and the channels
    without are bit-identical to the same Tuner built with no AGC anywhere."""
    tuner, bare = _tuner(rc, band, **options), _tuner(rc, band, agc=[False] * C, **options)
    want = [_expected(band, oracle, i, 3)[0] if WITH_AGC[i] else None for i in range(C)]
    worst = 0.0
    for buf in range(3):
        tuner.load(band["x"][buf])
        bare.load(band["x"][buf])
        got, ref = tuner.run_each(), bare.run_each()
        assert len(got) == C
        for i in range(C):
            if WITH_AGC[i]:
                assert got[i].shape == (A, 1)
                worst = max(worst, rel_err(got[i][:, 0], want[i][buf]))
                assert not np.array_equal(got[i], ref[i])
            else:
                assert np.array_equal(got[i], ref[i]), (buf, i)
    print("run_each", options, "worst rel err %.3g" % worst)
    assert worst <= TOL


def _uniform(rc, band):
    """All 24 channels of the band as USB with one AGC setting -- run_all needs one class, geometry and AGC setting.  Only
    the channels of USB_ROWS carry sideband stations the model knows as USB; the others are run and not compared."""
    t = rc.Tuner()
    for f in band["centres"]:
        t.add_channel(f, B, rc.USB(B, A, agc=rc.AGC(m.CHAIN_DECAY, floor=FLOOR["USB"])))
    t.request_bandwidth(float(N))
    return t


USB_ROWS = [i for i, k in enumerate(KINDS) if k == "USB"]       # the channels whose stations are sideband stations


def test_tuner_run_all_and_the_channel_objects_share_one_state(rc, oracle, band):
    """run_all over three buffers against the model; then, on a fresh tuner, demodulator.run(tuner.run(i)) on buffer 1
    and run_all on buffer 2: one state per channel, whoever runs it."""
    tuner = _uniform(rc, band)
    for buf in range(3):
        tuner.load(band["x"][buf])
        got = tuner.run_all()
        assert got.shape == (C, A, 1)
        for i in USB_ROWS:
            e = rel_err(got[i, :, 0], _expected(band, oracle, i, 3)[0][buf])
            assert e <= TOL, (buf, i, e)
    mixed = _uniform(rc, band)
    mixed.load(band["x"][0])
    i = USB_ROWS[1]
    ch = mixed.channels()[i]
    a0 = ch.demodulator.run(mixed.run(i))
    want, s_want = _expected(band, oracle, i, 2)
    assert rel_err(a0[:, 0], want[0]) <= TOL
    mixed.load(band["x"][1])
    a1 = mixed.run_all()
    assert rel_err(a1[i, :, 0], want[1]) <= TOL
    assert m.state_error(ch.demodulator.agc_state()[0], s_want) <= TOL
    other = USB_ROWS[2]                                  # a channel only run_all touched: its first buffer was buffer 1
    assert rel_err(a1[other, :, 0], _expected(band, oracle, other, 1, start=1)[0][0]) <= TOL
    mixed.reset_states()
    assert ch.demodulator.agc_state().tolist() == [-1.0]


def test_tuner_squelch_keeps_the_state_moving(rc, band):
    """Closed rows are exact zeros, open rows what they are without squelch, and the AGC state advances either way."""
    free, gated = _uniform(rc, band), _uniform(rc, band)
    free.load(band["x"][0])
    lv = free.levels()
    thr = np.where(np.arange(C) % 2 == 0, 0.5 * lv, 2.0 * lv).astype(np.float32)      # odd channels closed
    gated.set_squelch(thr)
    for buf in range(2):
        free.load(band["x"][buf])
        gated.load(band["x"][buf])
        a, b = free.run_all(), gated.run_all()
        mask = gated.open_mask()
        assert mask.tolist() == [i % 2 == 0 for i in range(C)]
        assert np.array_equal(a[mask], b[mask]) and not b[~mask].any()
    for i in (0, 1):
        assert np.array_equal(free.channels()[i].demodulator.agc_state(), gated.channels()[i].demodulator.agc_state())


def test_tuner_shard_and_lanes(rc, oracle, band):
    """After shard(first, count) run_all gives that range's channels, following the model with the state carried;
    Lanes(depth=2) over four buffers is bit-identical to the one-at-a-time loop."""
    from radiocore.tools import Lanes
    whole, part = _uniform(rc, band), _uniform(rc, band)
    part.shard(5, 9)
    want = []
    for buf in range(4):
        whole.load(band["x"][buf])
        part.load(band["x"][buf])
        want.append(whole.run_all())
        got = part.run_all()
        assert got.shape == (9, A, 1)
        for i in (5, 6, 7):                                  # the sideband stations inside the shard
            assert rel_err(got[i - 5, :, 0], _expected(band, oracle, i, 4)[0][buf]) <= TOL, (buf, i)
    lanes = Lanes(_uniform(rc, band), depth=2)
    tickets = [lanes.submit(x) for x in band["x"]]
    got = [lanes.result(t) for t in tickets]
    for buf in range(4):
        assert np.array_equal(got[buf], want[buf]), (buf, np.abs(got[buf] - want[buf]).max())
    mixed = Lanes(_tuner(rc, band), depth=2)               # run_each through the lanes: mixed classes, some with agc
    loop = _tuner(rc, band)
    tickets = [mixed.submit(x, each=True) for x in band["x"]]
    for buf, tk in enumerate(tickets):
        loop.load(band["x"][buf])
        for g, w in zip(mixed.result(tk), loop.run_each()):
            assert np.array_equal(g, w), buf


# ---- the example -------------------------------------------------------------------------------------------------------

def test_example_runs():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "radio-core_amd"), ROOT]))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ssb_agc.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "with agc" in out.stdout
