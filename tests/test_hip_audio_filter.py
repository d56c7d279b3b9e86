"""GPU: the per-channel audio filter (include/rcfm.h: rcfm_audio_filter_*, radiocore.AudioFilter, Tuner.set_audio_filter)
against tests/sos_model.py.

The primitive against the float64 recurrence on the same float32 input -- audio relative to the row's output peak, the
final state relative to its own largest entry, each within min(max(4 x the float32 yardstick's own error, 1e-6), 1e-4) --
over two calls with the state carried, mono and stereo; one row of 2 n against two calls of n; bit identity; select;
reset and the state's round trip; and the Tuner: tone bank, squelch, run_each, WBFM, the drain, lanes, a growing channel
list.  The yardstick is a float32 recurrence in Python and costs seconds per case: the bound is never below 1e-6, so it
is evaluated only where an error is above that (the float64 block model reads 5e-8: nowhere, as measured).

Worst figures measured on MI355X are recorded in DESIGN.md section 3.18.
"""

import ctypes
import importlib.util
import os

import numpy as np
import pytest

import sos_model as m
import workloads
from conftest import ROOT, have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

_dp = ctypes.POINTER(ctypes.c_double)
ERR_INDEX = -2


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def hip(rc):
    from radiocore._internal import hip
    return hip


@pytest.fixture(scope="module")
def af(rc):
    from radiocore.tools import audiofilter
    return audiofilter


class _Filter:
    """One rcfm_audio_filter handle."""

    def __init__(self, hip, C, ch, sos):
        self.hip, self.C, self.ch, self.S = hip, C, ch, len(sos)
        sos = np.ascontiguousarray(sos, dtype=np.float64)
        out = ctypes.c_void_p()
        hip.check(hip.lib().rcfm_audio_filter_create(C, ch, self.S, sos.ctypes.data_as(_dp), ctypes.byref(out)))
        self.handle = hip.Handle(out, hip.lib().rcfm_audio_filter_destroy)

    def run(self, x, first=0, out=None, select=None):
        """x: a device tensor [count, n] or [count, n, ch] -> the filtered tensor (a new one unless `out` is given)."""
        hip = self.hip
        out = hip.torch().empty_like(x) if out is None else out
        hip.check(hip.lib().rcfm_audio_filter_run(self.handle.value, first, int(x.shape[0]), int(x.shape[1]), hip.ptr(x),
                                                  hip.ptr(out), hip.ptr(select) if select is not None else None, hip.stream()))
        return out

    def state(self):
        s = np.zeros((self.C, self.ch, self.S, 2))
        self.hip.check(self.hip.lib().rcfm_audio_filter_get_state(self.handle.value, s.ctypes.data_as(_dp), self.hip.stream()))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, dtype=np.float64)
        assert s.shape == (self.C, self.ch, self.S, 2)
        self.hip.check(self.hip.lib().rcfm_audio_filter_set_state(self.handle.value, s.ctypes.data_as(_dp), self.hip.stream()))

    def reset(self):
        self.hip.check(self.hip.lib().rcfm_audio_filter_reset(self.handle.value, self.hip.stream()))


def _dev(hip, a):
    return hip.to_device(np.array(a, dtype=np.float32, order="C"))          # a copy: the model's arrays are read-only


def _legs(a, ch):
    """[3][...] per row -> [3][ch][...] per row and leg, as m.stereo lays the inputs out."""
    return m.stereo_of(a) if ch == 2 else np.asarray(a)[:, None]


def _within(err, yard):
    """err <= bound(yardstick's error); `yard` is a function, asked only where the bound's floor does not settle it."""
    return err <= m.FLOOR or err <= m.bound(yard())


# ---- the primitive -----------------------------------------------------------------------------------------------------

WORST = {}


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n", m.SIZES)
def test_primitive_against_float64(hip, n, ch):
    """Two calls with the state carried from zero, three rows over three decades of level (noise on a DC level, an 88.5 Hz
    tone under noise, voice-band noise); stereo: the right leg holds another row."""
    for name in m.filters(n):
        ref = m.reference(name, n)
        f = _Filter(hip, 3, ch, ref["sos"])
        assert not f.state().any()
        for call in range(2):
            x = ref["x"][call]
            got = hip.to_host(f.run(_dev(hip, m.stereo(x) if ch == 2 else x))).reshape(3, n, ch)
            st = f.state()
            want, s_want = _legs(ref["audio"][call], ch), _legs(ref["state"][call], ch)
            for r in range(3):
                for leg in range(ch):
                    row = (r + leg) % 3                      # the row of the model this leg carries
                    ea = m.audio_error(got[r, :, leg], want[r, leg])
                    es = m.state_error(st[r, leg], s_want[r, leg])
                    key = (name, ch)
                    WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0, 0.0)), (ea, es)))
                    assert _within(ea, lambda: m.yard_errors(name, n, call)[0][row]), (name, call, r, leg, ea)
                    assert _within(es, lambda: m.yard_errors(name, n, call)[1][row]), (name, call, r, leg, es)
        print("n=%d ch=%d %s: worst so far audio %.3g state %.3g" % ((n, ch, name) + WORST[(name, ch)]))


def test_one_row_of_2n_against_two_calls_of_n(hip):
    n = 8000
    for name in ("voice_nfm", "elliptic"):
        sos = m.filters(n)[name]
        x = np.concatenate([m.rows(n, 0), m.rows(n, 1)], axis=1)
        one, two = _Filter(hip, 3, 1, sos), _Filter(hip, 3, 1, sos)
        a1 = hip.to_host(one.run(_dev(hip, x)))
        a2 = np.concatenate([hip.to_host(two.run(_dev(hip, x[:, :n]))), hip.to_host(two.run(_dev(hip, x[:, n:])))], axis=1)
        for r in range(3):
            want, s_want = m.truth(sos, x[r])

            def yard():
                y, st = m.yardstick(sos, x[r])
                return max(m.audio_error(y[0], want), m.state_error(st[0], s_want))
            for what, got, f in (("one call", a1, one), ("two calls", a2, two)):
                ea, es = m.audio_error(got[r], want), m.state_error(f.state()[r, 0], s_want)
                print(name, what, "row", r, "audio %.3g state %.3g" % (ea, es))
                assert _within(ea, yard) and _within(es, yard)
            assert _within(m.audio_error(a1[r], a2[r]), yard)


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n", [8000, 8001])
def test_bit_identity(hip, n, ch):
    """Run to run, on a second stream, rows 1 - 2 alone against rows 1 - 2 of three, in place against out of place, from a
    row base that is 4 but not 16 bytes aligned (4-byte accesses instead of 16-byte ones), select NULL against all ones --
    audio and state, from a state that is not at rest."""
    t = hip.torch()
    sos = m.filters(8000)["voice_nfm"]
    x = m.rows(n, 0, rate=8000)
    x = m.stereo(x) if ch == 2 else x
    s0 = np.random.default_rng(5).standard_normal((3, ch, len(sos), 2)) * 1e-3

    def run(rows=slice(0, 3), first=0, in_place=False, shift=0, select=None):
        f = _Filter(hip, 3, ch, sos)
        f.set_state(s0)
        xx = x[rows]
        if shift:
            pad = t.zeros(xx.size + shift, dtype=t.float32, device="cuda")
            src = pad[shift:].view(xx.shape)
            src.copy_(_dev(hip, xx))
        else:
            src = _dev(hip, xx)
        out = f.run(src, first=first, out=src if in_place else None, select=select)
        return hip.to_host(out), f.state()

    a0, s_0 = run()
    assert not np.array_equal(s_0, s0)
    a1, s_1 = run()
    assert np.array_equal(a0, a1) and np.array_equal(s_0, s_1)
    with t.cuda.stream(t.cuda.Stream()):
        a2, s_2 = run()
        t.cuda.current_stream().synchronize()
    assert np.array_equal(a0, a2) and np.array_equal(s_0, s_2)
    a3, s_3 = run(rows=slice(1, 3), first=1)
    assert np.array_equal(a0[1:], a3) and np.array_equal(s_0[1:], s_3[1:]) and np.array_equal(s_3[0], s0[0])
    a4, s_4 = run(in_place=True)
    assert np.array_equal(a0, a4) and np.array_equal(s_0, s_4)
    for shift in (1, 2, 3):
        a5, s_5 = run(shift=shift)
        assert np.array_equal(a0, a5) and np.array_equal(s_0, s_5), shift
    a6, s_6 = run(select=t.ones(3, dtype=t.uint8, device="cuda"))
    assert np.array_equal(a0, a6) and np.array_equal(s_0, s_6)


@pytest.mark.parametrize("ch", [1, 2])
def test_select_leaves_a_row_and_its_state_alone(hip, ch):
    t = hip.torch()
    n = 8192
    sos = m.filters(n)["highpass"]
    x = m.rows(n, 0)
    x = m.stereo(x) if ch == 2 else x
    s0 = np.random.default_rng(6).standard_normal((3, ch, len(sos), 2)) * 1e-3
    sel = t.tensor([1, 0, 1], dtype=t.uint8, device="cuda")
    whole, part, place = (_Filter(hip, 3, ch, sos) for _ in range(3))
    for f in (whole, part, place):
        f.set_state(s0)
    want = hip.to_host(whole.run(_dev(hip, x)))
    got = hip.to_host(part.run(_dev(hip, x), select=sel))
    src = _dev(hip, x)
    same = hip.to_host(place.run(src, out=src, select=sel))
    for a, f in ((got, part), (same, place)):
        assert np.array_equal(a[1].view(np.uint32), x[1].view(np.uint32))           # the input, bit for bit
        assert np.array_equal(a[[0, 2]], want[[0, 2]])
        st = f.state()
        assert np.array_equal(st[1], s0[1]) and np.array_equal(st[[0, 2]], whole.state()[[0, 2]])


def test_reset_state_round_trip_and_index_refusals(hip):
    n = 1001
    sos = m.filters(n)["highpass"]
    f = _Filter(hip, 3, 2, sos)
    x0, x1 = (_dev(hip, m.stereo(m.rows(n, c))) for c in range(2))
    a0 = hip.to_host(f.run(x0))
    saved = f.state()
    assert saved.any()
    a1 = hip.to_host(f.run(x1))
    assert not np.array_equal(f.state(), saved)
    f.set_state(saved)
    assert np.array_equal(f.state(), saved)
    assert np.array_equal(hip.to_host(f.run(x1)), a1)        # the next buffer, bit for bit
    f.reset()
    assert not f.state().any()
    assert np.array_equal(hip.to_host(f.run(x0)), a0)
    lib = hip.lib()
    for first, count in ((-1, 1), (3, 1), (1, 3), (0, 4)):
        before = f.state()
        status = lib.rcfm_audio_filter_run(f.handle.value, first, count, n, hip.ptr(x0), hip.ptr(x0), None, hip.stream())
        assert status == ERR_INDEX and b"channels" in lib.rcfm_last_error()
        assert np.array_equal(f.state(), before)
    with pytest.raises(IndexError):
        f.run(x0, first=2)


def test_the_fence_orders_two_streams(hip):
    """One handle, consecutive buffers on alternating streams with set_fence: what one stream gives."""
    t = hip.torch()
    n = 48000
    sos = m.filters(n)["voice_nfm"]
    xs = [_dev(hip, m.rows(n, c)) for c in range(4)]
    loop = _Filter(hip, 3, 1, sos)
    want = [hip.to_host(loop.run(x)) for x in xs]
    fenced = _Filter(hip, 3, 1, sos)
    hip.check(hip.lib().rcfm_audio_filter_set_fence(fenced.handle.value, 1))
    streams = [t.cuda.Stream(), t.cuda.Stream()]
    t.cuda.synchronize()
    outs = []
    for i, x in enumerate(xs):
        with t.cuda.stream(streams[i % 2]):
            outs.append(fenced.run(x))
    t.cuda.synchronize()
    for i in range(4):
        assert np.array_equal(hip.to_host(outs[i]), want[i]), i
    assert np.array_equal(fenced.state(), loop.state())
    hip.check(hip.lib().rcfm_audio_filter_set_fence(fenced.handle.value, 0))


def test_audio_filter_object_runs_in_place(hip, af):
    """radiocore.AudioFilter.run: in place on the current stream with a handle of its own per (channels, legs, A)."""
    n = 8000
    x = m.rows(n, 0)
    filt = af.AudioFilter.highpass(300.0)
    direct = _Filter(hip, 3, 1, filt.sections(n))
    want = [hip.to_host(direct.run(_dev(hip, m.rows(n, c)))) for c in range(2)]
    for c in range(2):
        d = _dev(hip, m.rows(n, c))
        assert filt.run(d) is d
        assert np.array_equal(hip.to_host(d), want[c])
    filt.reset()
    d = _dev(hip, x)[:, :, None].contiguous()
    assert np.array_equal(hip.to_host(filt.run(d))[:, :, 0], want[0])
    with pytest.raises(ValueError):
        filt.run(_dev(hip, x[:, :500]))                      # no design for a 300 Hz corner at a rate of 500
    with pytest.raises(ValueError):
        filt.run(_dev(hip, x).double())


# ---- through the Tuner ---------------------------------------------------------------------------------------------

RATE, CHANNELS, WANTED, RATIO = 1_000_000, 16, 88.5, 0.01


@pytest.fixture(scope="module")
def pmr():
    """examples/pmr_audio_filter.py (and, through it, the stations of examples/pmr_tone_squelch.py)."""
    spec = importlib.util.spec_from_file_location("pmr_audio_filter", os.path.join(ROOT, "examples", "pmr_audio_filter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _centres(pmr, channels=CHANNELS):
    return [446_006_250.0 + pmr.pmr.CHANNEL * i for i in range(channels)]


def _tuner(rc, pmr, channels=CHANNELS, kinds=None):
    t = rc.Tuner()
    for i, f in enumerate(_centres(pmr, channels)):
        t.add_channel(f, pmr.pmr.CHANNEL, getattr(rc, kinds[i] if kinds else "FM")(pmr.pmr.CHANNEL, pmr.pmr.AUDIO))
    t.request_bandwidth(float(RATE))
    return t


@pytest.fixture(scope="module")
def band(rc, pmr):
    """Three buffers of the 16-channel PMR band: five stations each, two of them with the wanted tone; channel 3 carries
    one in every buffer.  With the unfiltered audio of every channel (FM carries no state) -- computed once, read-only."""
    t = _tuner(rc, pmr)
    rng = np.random.default_rng(11)
    plans, bufs, plain = [], [], []
    for b in range(3):
        others = [int(i) for i in rng.choice([c for c in range(CHANNELS) if c != 3], 4, replace=False)]
        plan = dict(zip([3] + others, [WANTED, WANTED, 100.0, 123.0, 71.9]))
        x = pmr.pmr.band(RATE, _centres(pmr), t.input_frequency, plan, rng)
        t.load(x)
        audio = t.run_all()
        audio.setflags(write=False)
        plans.append(plan), bufs.append(x), plain.append(audio)
    return dict(plans=plans, bufs=bufs, plain=plain)


def _model(sos, rows_per_buffer):
    """([audio float64], [state]) per buffer of one channel's unfiltered rows through the truth, the state carried from zero."""
    st, out, states = None, [], []
    for row in rows_per_buffer:
        y, st = m.truth(sos, row, st)
        out.append(y)
        states.append(st.copy())
    return out, states


def _check(got, sos, rows_per_buffer, what):
    """The last buffer's `got` against the model of the rows so far, within the primitive's bound: the yardstick (from the
    truth's state before that buffer) is asked only where the bound's floor does not settle it.  -> the error."""
    want, states = _model(sos, rows_per_buffer)
    e = m.audio_error(got, want[-1])
    before = states[-2][None] if len(states) > 1 else None
    print("%s: %.3g" % (what, e))
    assert _within(e, lambda: m.audio_error(m.yardstick(sos, rows_per_buffer[-1], before)[0][0], want[-1])), (what, e)
    return e


def test_tuner_tone_squelch_and_voice_filter(rc, af, pmr, band):
    """set_tones(want=88.5) with and without set_audio_filter(VOICE_NFM) over two buffers: tone_power() bit for bit, the
    same mask, closed rows exact zeros, open rows the model's filter of the unfiltered audio with the state carried from
    the first buffer on (open or not), and the hum gone.  The hum is read as the level of the row's 88.5 Hz component (a
    Hann-windowed projection, what the tone bank's P is): it drops by the filter's own attenuation there, less 3 dB.  (Its
    share P / E of the row's power drops by less than that, since the de-emphasis takes 14 dB off the speech as well.)"""
    from radiocore.tools import tones
    sos = af.VOICE_NFM.sections(pmr.pmr.AUDIO)
    bare, voiced = _tuner(rc, pmr), _tuner(rc, pmr)
    for t in (bare, voiced):
        t.set_tones(rc.ToneBank(tones.CTCSS), want=WANTED, ratio=RATIO)
    voiced.set_audio_filter(af.VOICE_NFM)
    atten = pmr.attenuation_db(af.VOICE_NFM)
    assert atten > 40.0
    worst = 0.0
    for b in range(2):
        bare.load(band["bufs"][b])
        voiced.load(band["bufs"][b])
        a, v = bare.run_all(), voiced.run_all()
        for x, y in zip(bare.tone_power(), voiced.tone_power()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        mask = voiced.open_mask()
        assert np.array_equal(mask, bare.open_mask())
        assert sorted(np.flatnonzero(mask)) == sorted(c for c, f in band["plans"][b].items() if f == WANTED)
        assert not v[~mask].any()
        for c in np.flatnonzero(mask):
            assert np.array_equal(a[c], band["plain"][b][c])
            worst = max(worst, _check(v[c, :, 0], sos, [band["plain"][k][c, :, 0] for k in range(b + 1)], "buffer %d channel %d" % (b, c)))
            before, after = pmr.hum_db(a[c, :, 0]), pmr.hum_db(v[c, :, 0])
            print("buffer %d channel %d: hum %.1f dB -> %.1f dB (the filter takes %.1f dB)" % (b, c, before, after, atten))
            assert before - after >= atten - 3.0
    print("open rows against the model: worst %.3g" % worst)
    voiced.set_audio_filter(None)
    voiced.set_tones(None)
    voiced.load(band["bufs"][0])
    assert np.array_equal(voiced.run_all().view(np.uint32), band["plain"][0].view(np.uint32))     # the parent's audio


def test_tuner_state_moves_on_closed_channels_and_reset_states(rc, af, pmr, band):
    """A level squelch of +inf closes every row: exact zeros, and the filter's states advance all the same -- the third
    buffer, squelch off, follows the model from the first one on.  reset_states() puts the filter at rest."""
    sos = af.VOICE_NFM.sections(pmr.pmr.AUDIO)
    t = _tuner(rc, pmr)
    t.set_audio_filter(af.VOICE_NFM)
    t.set_squelch(np.inf)
    for b in range(2):
        t.load(band["bufs"][b])
        assert not t.run_all().any() and not t.open_mask().any()
    t.set_squelch(None)
    t.load(band["bufs"][2])
    got = t.run_all()
    for c in (3, 0):
        _check(got[c, :, 0], sos, [band["plain"][k][c, :, 0] for k in range(3)], "channel %d, third buffer" % c)
    want, _ = _model(sos, [band["plain"][k][3, :, 0] for k in range(3)])
    rest, _ = _model(sos, [band["plain"][2][3, :, 0]])
    assert m.audio_error(rest[0], want[2]) > 1e-4                               # the carried state matters
    t.reset_states()
    t.load(band["bufs"][0])
    again = t.run_all()
    fresh = _tuner(rc, pmr)
    fresh.set_audio_filter(af.VOICE_NFM)
    fresh.load(band["bufs"][0])
    assert np.array_equal(again, fresh.run_all())


def test_tuner_selected_channels_and_run_each_over_fm_and_am(rc, af, pmr, band):
    """run_each over a group of FM and a group of AM channels (both 8000 samples of audio: one handle, addressed by
    channel index), the filter on every second channel only; the others are the unfiltered audio bit for bit."""
    kinds = ["FM"] * 8 + ["AM"] * 8
    sel = np.arange(CHANNELS) % 2 == 0
    bare, t = _tuner(rc, pmr, kinds=kinds), _tuner(rc, pmr, kinds=kinds)
    t.set_audio_filter(af.VOICE_AM, channels=sel)
    sos = af.VOICE_AM.sections(pmr.pmr.AUDIO)
    rows = {c: [] for c in (0, 2, 8, 14)}
    for b in range(2):
        bare.load(band["bufs"][b])
        t.load(band["bufs"][b])
        plain, got = bare.run_each(), t.run_each()
        assert len(got) == CHANNELS and all(g.shape == (pmr.pmr.AUDIO, 1) for g in got)
        for c in range(CHANNELS):
            if not sel[c]:
                assert np.array_equal(got[c].view(np.uint32), plain[c].view(np.uint32)), (b, c)
        for c in rows:
            rows[c].append(plain[c][:, 0])
            _check(got[c][:, 0], sos, rows[c], "run_each buffer %d channel %d (%s)" % (b, c, kinds[c]))
    assert len(t._afilt_handles) == 1
    whole = _tuner(rc, pmr)                                  # run_all gives what run_each gives
    whole.set_audio_filter(af.VOICE_AM, channels=sel)
    each = _tuner(rc, pmr)
    each.set_audio_filter(af.VOICE_AM, channels=sel)
    whole.load(band["bufs"][0])
    each.load(band["bufs"][0])
    assert np.array_equal(whole.run_all(), np.stack(each.run_each()))


def test_tuner_wbfm_both_legs(rc, af):
    """One WBFM channel: interleaved stereo, each leg a row of its own with its own state, over two buffers."""
    bw, A, n = 60000, 12000, 600000
    centres = workloads.channel_grid(1, bw)
    tuners = []
    for voice in (None, af.VOICE_NFM):
        t = rc.Tuner()
        t.add_channel(centres[0], bw, rc.WBFM(bw, A))
        t.request_bandwidth(float(n))
        t.set_audio_filter(voice)
        tuners.append(t)
    x = workloads.wideband(n, tuners[0].input_frequency, centres, bw, gain=0.5)
    sos = af.VOICE_NFM.sections(A)
    plain = []
    for b in range(2):
        out = []
        for t in tuners:
            t.load(x)
            out.append(t.run_all())
        assert out[1].shape == (1, A, 2)
        plain.append(out[0])
        for leg in range(2):
            _check(out[1][0, :, leg], sos, [p[0, :, leg] for p in plain], "WBFM buffer %d leg %d" % (b, leg))
    assert not np.array_equal(out[1][0, :, 0], out[1][0, :, 1])


def test_tuner_packed_drain_and_lanes(rc, af, pmr, band):
    """run_all_packed with a Drain publishes the filtered open rows; Lanes(depth=2) over three buffers is bit-identical to
    the one-buffer loop, audio, mask and tone powers."""
    from radiocore.tools import Drain, Lanes, tones

    def make():
        t = _tuner(rc, pmr)
        t.set_tones(rc.ToneBank(tones.CTCSS), want=WANTED, ratio=RATIO)
        t.set_audio_filter(af.VOICE_NFM)
        return t
    loop = make()
    expect = []
    for x in band["bufs"]:
        loop.load(x)
        audio = loop.run_all()
        expect.append((audio, loop.open_mask(), loop.tone_power()))
    packed = make()
    drain = Drain(CHANNELS, (pmr.pmr.AUDIO, 1), "float32", depth=2)
    pcm = rc.PCM("float32")
    for b, x in enumerate(band["bufs"]):
        packed.load(x)
        packed.run_all_packed(pcm, drain=drain)
        with drain.next() as (index, rows):
            assert index.tolist() == np.flatnonzero(expect[b][1]).tolist()
            assert np.array_equal(rows, expect[b][0][expect[b][1]])
    drain.close()
    lanes = Lanes(make(), depth=2)
    tickets = [lanes.submit(x) for x in band["bufs"]]
    for (audio, mask, (P, E)), ticket in zip(expect, tickets):
        got, got_mask, (gP, gE) = lanes.result(ticket, open_mask=True, tones=True)
        assert np.array_equal(got.view(np.uint32), audio.view(np.uint32))
        assert np.array_equal(got_mask, mask) and np.array_equal(gP, P) and np.array_equal(gE, E)


def test_tuner_add_channel_keeps_the_states(rc, af, pmr, band):
    """A seventeenth channel after the first buffer: the handle is made anew for 17 channels and the sixteen states move
    into it -- channel 3 follows the model from the first buffer on, the new channel starts at rest."""
    sos = af.VOICE_NFM.sections(pmr.pmr.AUDIO)
    t = _tuner(rc, pmr)
    t.set_audio_filter(af.VOICE_NFM)
    t.load(band["bufs"][0])
    t.run_all()
    extra = _centres(pmr, CHANNELS + 1)[-1]
    bare = _tuner(rc, pmr, CHANNELS + 1)
    t.add_channel(extra, pmr.pmr.CHANNEL, rc.FM(pmr.pmr.CHANNEL, pmr.pmr.AUDIO))
    t.request_bandwidth(float(RATE))
    assert t.input_frequency == bare.input_frequency
    rng = np.random.default_rng(12)
    x = pmr.pmr.band(RATE, _centres(pmr, CHANNELS + 1), t.input_frequency, {3: WANTED, 16: 100.0, 7: 123.0}, rng)
    bare.load(x)
    t.load(x)
    plain, got = bare.run_all(), t.run_all()
    assert got.shape == (CHANNELS + 1, pmr.pmr.AUDIO, 1)
    for c, history in ((3, [band["plain"][0][3, :, 0]]), (7, [band["plain"][0][7, :, 0]]), (16, [])):
        _check(got[c, :, 0], sos, history + [plain[c, :, 0]], "after add_channel, channel %d" % c)
    rest, _ = _model(sos, [plain[3, :, 0]])
    assert m.audio_error(rest[0], _model(sos, [band["plain"][0][3, :, 0], plain[3, :, 0]])[0][1]) > 1e-4     # the state matters
    with pytest.raises(ValueError):
        t.reset()                                            # as the reference: min() of nothing
    assert not t._afilt_handles


def test_pmr_audio_filter_example(pmr):
    """examples/pmr_audio_filter.py: its own assertions hold."""
    results = pmr.run(channels=16, rate=1_000_000, seconds=2)
    assert len(results) == 2
    pmr.check(results)
