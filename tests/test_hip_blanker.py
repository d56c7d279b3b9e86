"""GPU: the noise blanker (rcfm_blanker_create / _run / _last, NoiseBlanker, Tuner.set_blanker) against its definition in
include/rcfm.h, evaluated by tests/blanker_model.py.

Everything is compared exactly -- the hit mask, the stats and the bits of the output -- except the thresholds, which may be
one float32 ulp from the model's: the one tolerance, for the order of the block sums.  (The header pins that order to a
pairwise tree the model builds too, and on an MI355X every threshold of every case came out 0 ulp away; the test prints the
figure per case.)  tests/test_blanker_model.py shows that no input used here has a sample that close to its threshold, so
the tolerance cannot change a hit.  Every run writes into a buffer with guard bytes on both sides, and the guards are
checked: nothing is stored outside [out, out + n samples).

Shapes: n in {1, 63, 64, 65, 1000, 4096, 4097, 12 289, 100 003} x L in {64, 256, 4096} x W in {0, 1, 4, 8} (so nb = 1 and
nb < 2 W + 1 occur), the four formats, the guards (H, R) in {(0, 0), (0, 5), (8, 8), (1000, 24)} and both modes taken in
turn; pulses at sample 0, n - 1, 4095 and 4096 (the tile edge), a block edge, two closer than the guard; 5000 hits in a
row (a whole tile on the slow branch); no hit at all; full-scale integer codes; a NaN and an Inf."""

import ctypes
import importlib.util
import os

import numpy as np
import pytest

import blanker_model as bm
from conftest import ROOT, have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ERR_ARG = -4
FMT = {np.dtype("complex64"): 0, np.dtype("int16"): 1, np.dtype("int8"): 2, np.dtype("uint8"): 3}
ELEM = {0: 8, 1: 4, 2: 2, 3: 2}
GUARD = 64                      # bytes in front of and behind every device buffer of a run
ODD_RAMP = np.array([0.5, 0.25, 1.0, 0.0, 0.75, 0.125, 0.9, 0.3, 0.6], np.float32)      # not monotonic; holds a 1 and a 0


def _case_id(c):
    return "%s-n%d-L%d-W%d-H%d-R%d-m%d" % c[:7]


def special_cases():
    """(name, x, kw) beyond the shape table."""
    out = []
    for k, fmt in enumerate(bm.FORMATS):
        for hold, R in ((8, 8), (1000, 24)):
            case = (fmt, 12289, 256, 1, hold, R, bm.ABSOLUTE, 300 + k)
            out.append(("stretch-" + _case_id(case),) + bm.case_input(case, stretch=True))
        case = (fmt, 12289, 4096, 8, 1000, 24, bm.MEDIAN, 310 + k)
        out.append(("stretch-" + _case_id(case),) + bm.case_input(case, stretch=True))
        for mode in (bm.MEDIAN, bm.ABSOLUTE):
            case = (fmt, 12289, 256, 4, 8, 8, mode, 320 + k)
            x = bm.make_input(fmt, 12289, case[7])
            out.append(("nohit-" + _case_id(case), x, bm.case_input(case)[1]))
    case = ("cf32", 4097, 64, 1, 0, 9, bm.MEDIAN, 330)
    x, kw = bm.case_input(case)
    kw["ramp"] = ODD_RAMP
    out.append(("oddramp-" + _case_id(case), x, kw))
    case = ("cf32", 4097, 256, 4, 3, 5, bm.MEDIAN, 331)      # (nine blocks to a median: two non-finite levels do not reach it)
    x, kw = bm.case_input(case)
    x = x.copy()
    x[100] = complex(np.nan, 1.0)               # far from every hit: copied bit for bit
    x[259] = complex(2.0, np.nan)               # in the hold of the pulse at 256
    x[250] = complex(np.nan, np.nan)            # in the ramp of the pulse at 255
    x[2000] = complex(np.inf, 0.0)              # a hit; its block's level counts as +inf
    x[3000] = complex(-0.0, -0.0)
    out.append(("nonfinite-" + _case_id(case), x, kw))
    return out


def tuner_buffer(fmt, N, seed):
    rng = np.random.default_rng(seed)
    return bm.make_input(fmt, N, seed, np.sort(rng.choice(N, 60, replace=False)))


def tuner_kw(N):
    return dict(block=4096, span=4, mode=bm.MEDIAN, value=10.0 ** 1.2, hold=int(round(2e-5 * N)),
                ramp=bm.raised_cosine(int(round(1e-5 * N))))


TUNER_SIZES = (240_000, 2_400_000)


def exact_inputs():
    """Every (name, x, kw) this file compares exactly with the model (tests/test_blanker_model.py checks each is robust)."""
    for case in bm.shape_cases():
        yield (_case_id(case),) + bm.case_input(case)
    for item in special_cases():
        yield item
    for N in TUNER_SIZES:
        for k, fmt in enumerate(("cf32", "cs16", "cu8")):
            yield "tuner-%s-%d" % (fmt, N), tuner_buffer(fmt, N, 400 + k), tuner_kw(N)
    for k in range(3):
        yield "lanes-%d" % k, tuner_buffer("cf32", TUNER_SIZES[0], 410 + k), tuner_kw(TUNER_SIZES[0])


@pytest.fixture(scope="module")
def rc():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    return radiocore


@pytest.fixture(scope="module")
def hip(rc):
    from radiocore._internal import hip
    return hip


def _create(hip, n_max, kw):
    ramp = np.ascontiguousarray(kw["ramp"], np.float32)
    h = ctypes.c_void_p()
    hip.check(hip.lib().rcfm_blanker_create(n_max, kw["block"], kw["span"], kw["mode"], float(kw["value"]), kw["hold"],
                                            ramp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if ramp.size else None,
                                            int(ramp.size), ctypes.byref(h)))
    return hip.Handle(h, hip.lib().rcfm_blanker_destroy)


class Device:
    """One buffer of `nbytes` on the device, GUARD bytes of 0xA5 each side, its first byte `shift` bytes behind a 256-byte
    boundary."""

    def __init__(self, hip, nbytes, shift=0):
        t = hip.torch()
        self.t, self.nbytes, self.lo = t, nbytes, GUARD + shift
        self.raw = t.full((nbytes + 2 * GUARD + shift + 16,), 0xA5, dtype=t.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = ctypes.c_void_p(self.raw.data_ptr() + self.lo)

    def put(self, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert b.shape[0] == self.nbytes
        if self.nbytes:
            self.raw[self.lo:self.lo + self.nbytes].copy_(self.t.from_numpy(b.copy()))
        return self

    def fill(self, x):
        """NaN for complex64, 0x55 bytes for the integer formats."""
        if x.dtype == np.complex64:
            return self.put(np.full(x.shape, np.nan + 1j * np.nan, np.complex64))
        return self.put(np.full(x.shape, 0x55, np.uint8).view(x.dtype) if x.dtype != np.int16
                        else np.full(x.shape, 0x5555, np.int16))

    def get(self, like):
        whole = self.raw.cpu().numpy()
        assert np.all(whole[:self.lo] == 0xA5) and np.all(whole[self.lo + self.nbytes:] == 0xA5), "a store outside the buffer"
        return whole[self.lo:self.lo + self.nbytes].copy().view(like.dtype).reshape(like.shape)


def run_device(hip, x, kw, in_place=False, shift_in=0, shift_out=0, handle=None, stream=None):
    """(out, input afterwards, t, mask words, stats) of one rcfm_blanker_run."""
    t = hip.torch()
    n = x.shape[0]
    fmt = FMT[x.dtype]
    h = handle if handle is not None else _create(hip, max(n, 1), kw)
    src = Device(hip, x.nbytes, shift_in).put(x)
    dst = src if in_place else Device(hip, x.nbytes, shift_out).fill(x)
    stats = t.full((2,), -7, dtype=t.int64, device="cuda")
    s = stream if stream is not None else t.cuda.current_stream()
    t.cuda.synchronize()
    hip.check(hip.lib().rcfm_blanker_run(h.value, fmt, n, src.ptr, dst.ptr, hip.ptr(stats), ctypes.c_void_p(s.cuda_stream)))
    s.synchronize()
    tp, mp, nb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    hip.check(hip.lib().rcfm_blanker_last(h.value, ctypes.byref(tp), ctypes.byref(mp), ctypes.byref(nb)))
    assert nb.value == -(-n // kw["block"])
    thr = np.empty(nb.value, np.float32)
    words = np.empty(-(-n // 4096) * 128, np.uint32)
    hip.check(hip.lib().rcfm_memcpy_d2h(thr.ctypes.data_as(ctypes.c_void_p), tp, thr.nbytes, None))
    hip.check(hip.lib().rcfm_memcpy_d2h(words.ctypes.data_as(ctypes.c_void_p), mp, words.nbytes, None))
    hip.check(hip.lib().rcfm_stream_sync(None))
    return dst.get(x), src.get(x), thr, words, tuple(int(v) for v in stats.cpu().numpy())


def ulps(a, b):
    """Largest distance in float32 steps between two arrays of non-negative thresholds (+inf equal to +inf only)."""
    a, b = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.max(np.abs(a - b))) if a.size else 0


def check(hip, name, x, kw, want=None, **how):
    want = want if want is not None else bm.blank(x, **kw)
    out, src, thr, words, stats = run_device(hip, x, kw, **how)
    worst = ulps(thr, want.t)
    print("%s %s: %d hits, %d blanked, thresholds within %d ulp" % (name, how, stats[0], stats[1], worst))
    assert worst <= 1, name
    assert np.array_equal(words, bm.mask_words(want.hit)), name
    assert stats == want.stats, name
    assert out.tobytes() == want.out.tobytes(), name
    if not how.get("in_place"):
        assert src.tobytes() == np.ascontiguousarray(x).tobytes(), name
    return want


@pytest.mark.parametrize("n", bm.SHAPES)
def test_every_shape_block_and_span_out_of_place_and_in_place(hip, n):
    cases = [c for c in bm.shape_cases() if c[1] == n]
    assert len(cases) == len(bm.BLOCKS) * len(bm.SPANS)
    hits = 0
    for case in cases:
        x, kw = bm.case_input(case)
        want = check(hip, _case_id(case), x, kw)
        check(hip, _case_id(case), x, kw, want=want, in_place=True)
        hits += want.stats[0]
    assert hits > 0


@pytest.mark.parametrize("item", special_cases(), ids=lambda i: i[0])
def test_stretches_empty_buffers_odd_ramps_and_non_finite_samples(hip, item):
    name, x, kw = item
    want = check(hip, name, x, kw)
    check(hip, name, x, kw, want=want, in_place=True)
    if name.startswith("stretch") and kw["mode"] == bm.ABSOLUTE:
        assert want.stats[0] >= 5000 and want.hit[5000:10000].all()       # tile 1 is all hits: the slow branch, whole
    if name.startswith("nohit"):
        assert want.stats == (0, 0)
    if name.startswith("nonfinite"):
        assert want.hit[2000] and not want.hit[100] and np.isnan(want.out[100].real) and want.out[259] == 0
        assert np.isposinf(want.m[[0, 1, 2000 // kw["block"]]]).all() and np.isfinite(want.t).all()
        assert want.d[250] == 5 and np.isnan(want.out[250].real)
        assert np.signbit(want.out[3000].real)


def test_no_hit_in_place_leaves_every_bit(hip):
    """out == in without a hit: the buffer's bits are unchanged (nothing is stored: the guards and a NaN payload stay)."""
    x = bm.make_input("cf32", 12289, 340).copy()
    x.view(np.uint32)[2 * 777] = 0x7fc54321
    kw = bm.case_input(("cf32", 12289, 4096, 0, 8, 8, bm.ABSOLUTE, 0))[1]
    kw["value"] = 1e6
    out, _, _, words, stats = run_device(hip, x, kw, in_place=True)
    assert out.tobytes() == x.tobytes() and not words.any() and stats == (0, 0)


@pytest.mark.parametrize("fmt", list(bm.FORMATS))
def test_buffers_one_sample_off_a_16_byte_boundary_give_the_same_bits(hip, fmt):
    elem = ELEM[FMT[bm.FORMATS[fmt]]]
    for case in ((fmt, 12289, 256, 1, 1000, 24, bm.MEDIAN, 350), (fmt, 1000, 64, 4, 0, 5, bm.ABSOLUTE, 351),
                 (fmt, 100003, 4096, 1, 8, 8, bm.MEDIAN, 352)):
        x, kw = bm.case_input(case, stretch=case[1] == 12289)
        assert bm.robust(x, **kw)
        want = bm.blank(x, **kw)
        for how in (dict(shift_in=elem, shift_out=elem), dict(shift_in=elem), dict(shift_out=elem),
                    dict(shift_in=elem, in_place=True), dict(shift_in=16 - elem, shift_out=3 * elem)):
            check(hip, _case_id(case), x, kw, want=want, **how)


def test_repeats_on_one_stream_and_on_a_second_stream_give_the_same_bits(hip):
    t = hip.torch()
    case = ("cs16", 100003, 256, 4, 8, 8, bm.MEDIAN, 360)
    x, kw = bm.case_input(case, stretch=True)
    assert bm.robust(x, **kw)
    h = _create(hip, x.shape[0], kw)
    first = run_device(hip, x, kw, handle=h)
    other = t.cuda.Stream()
    for stream in (None, None, other, other, None):
        again = run_device(hip, x, kw, handle=h, stream=stream)
        for a, b in zip(first, again):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    check(hip, _case_id(case), x, kw)
    # a handle serves shorter buffers too, and nothing of a longer run is left in its mask
    short, _ = bm.case_input(("cs16", 1000, 256, 4, 8, 8, bm.MEDIAN, 361))
    want = bm.blank(short, **kw)
    out, _, thr, words, stats = run_device(hip, short, kw, handle=h)
    assert out.tobytes() == want.out.tobytes() and stats == want.stats and np.array_equal(words, bm.mask_words(want.hit))


def test_run_refuses_before_anything_is_launched(hip):
    lib = hip.lib()
    t = hip.torch()
    case = ("cs16", 4097, 256, 1, 8, 8, bm.MEDIAN, 370)
    x, kw = bm.case_input(case)
    n = x.shape[0]
    h = _create(hip, n, kw)
    src, dst = Device(hip, x.nbytes).put(x), Device(hip, x.nbytes).fill(x)
    big = Device(hip, 2 * x.nbytes).fill(np.concatenate([x, x]))
    stats = t.full((2,), -7, dtype=t.int64, device="cuda")
    sp = hip.ptr(stats)
    p = lambda d, off=0: ctypes.c_void_p(d.ptr.value + off)      # noqa: E731
    refused = [
        (None, 1, n, src.ptr, dst.ptr, sp), (h.value, 1, n, None, dst.ptr, sp), (h.value, 1, n, src.ptr, None, sp),
        (h.value, 1, -1, src.ptr, dst.ptr, sp), (h.value, 1, n + 1, src.ptr, dst.ptr, sp),
        (h.value, 4, n, src.ptr, dst.ptr, sp), (h.value, -1, n, src.ptr, dst.ptr, sp),
        (h.value, 1, n, p(src, 2), dst.ptr, sp), (h.value, 1, n, src.ptr, p(dst, 2), sp),          # one integer off
        (h.value, 1, n, p(src, 1), dst.ptr, sp), (h.value, 2, n, p(src, 1), dst.ptr, sp),          # one byte off
        (h.value, 3, n, src.ptr, p(dst, 1), sp), (h.value, 0, n // 2, p(src, 4), dst.ptr, sp),     # one float off
        (h.value, 1, n, src.ptr, dst.ptr, ctypes.c_void_p(sp.value + 4)),
        (h.value, 1, n, big.ptr, p(big, 4), sp), (h.value, 1, n, p(big, 4 * (n - 1)), big.ptr, sp),    # partial overlap
    ]
    for args in refused:
        assert lib.rcfm_blanker_run(*args, None) == ERR_ARG, args
    t.cuda.synchronize()
    assert src.get(x).tobytes() == x.tobytes()
    assert dst.get(x).tobytes() == np.full(x.shape, 0x5555, np.int16).tobytes()
    assert np.all(big.get(np.concatenate([x, x])) == 0x5555)
    assert stats.cpu().tolist() == [-7, -7]
    # n = 0: a no-op that zeroes stats
    assert lib.rcfm_blanker_run(h.value, 1, 0, src.ptr, dst.ptr, sp, None) == 0
    t.cuda.synchronize()
    assert stats.cpu().tolist() == [0, 0] and dst.get(x).tobytes() == np.full(x.shape, 0x5555, np.int16).tobytes()
    # adjacent buffers are not an overlap
    assert lib.rcfm_blanker_run(h.value, 1, n, big.ptr, p(big, 4 * n), sp, None) == 0
    t.cuda.synchronize()


# ---- NoiseBlanker and the Tuner -----------------------------------------------------------------------------------------

B, A = 25_000, 8_000


def _tuner(rc, N):
    tuner = rc.Tuner()
    for i in range(2):
        tuner.add_channel(100e6 + B * i, B, rc.AM(B, A))
    tuner.request_bandwidth(float(N))
    return tuner


def _spectrum(hip, tuner, N):
    X = ctypes.c_void_p()
    hip.check(hip.lib().rcfm_tuner_spectrum(tuner._handle.value, ctypes.byref(X)))
    out = np.empty(N, np.complex64)
    hip.torch().cuda.synchronize()
    hip.check(hip.lib().rcfm_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), X, out.nbytes, None))
    hip.check(hip.lib().rcfm_stream_sync(None))
    return out


def _blanker(rc):
    return rc.NoiseBlanker(threshold_db=12.0, hold=2e-5, ramp=1e-5)


_models = {}


def _model(fmt, N, seed):
    key = (fmt, N, seed)
    if key not in _models:
        x = tuner_buffer(fmt, N, seed)
        _models[key] = (x, bm.blank(x, **tuner_kw(N)))
    return _models[key]


@pytest.mark.parametrize("N", TUNER_SIZES)
def test_noise_blanker_run_equals_the_model_in_every_format(rc, hip, N):
    t = hip.torch()
    nb = _blanker(rc)
    H, ramp = nb.geometry(N)
    assert H == tuner_kw(N)["hold"] and np.array_equal(ramp, tuner_kw(N)["ramp"])
    for k, fmt in enumerate(("cf32", "cs16", "cu8")):
        x, want = _model(fmt, N, 400 + k)
        y, stats = nb.run(x, stats=True)
        assert isinstance(y, np.ndarray) and y.dtype == x.dtype and y.shape == x.shape
        assert y.tobytes() == want.out.tobytes() and stats == want.stats and stats[0] >= 60
        xd = t.from_numpy(x.copy()).cuda()
        yd = nb.run(xd)
        assert yd.data_ptr() != xd.data_ptr() and xd.cpu().numpy().tobytes() == x.tobytes()
        assert yd.cpu().numpy().tobytes() == want.out.tobytes()
        assert nb.run(xd, out=xd) is xd and xd.cpu().numpy().tobytes() == want.out.tobytes()
    with pytest.raises(ValueError):
        nb.run(xd, out=xd.reshape(-1)[1:-1].reshape(-1, 2))


@pytest.mark.parametrize("N", TUNER_SIZES)
def test_tuner_with_a_blanker_loads_the_blanked_buffer(rc, hip, N):
    t = hip.torch()
    nb = _blanker(rc)
    plain, tuner = _tuner(rc, N), _tuner(rc, N)
    x, want = _model("cf32", N, 400)
    plain.load(x)
    never = _spectrum(hip, plain, N)
    plain.load(want.out)
    ref = _spectrum(hip, plain, N)
    plain.load(nb.run(x))
    assert _spectrum(hip, plain, N).tobytes() == ref.tobytes()
    assert ref.tobytes() != never.tobytes()
    tuner.set_blanker(nb)
    tuner.load(x)
    assert _spectrum(hip, tuner, N).tobytes() == ref.tobytes()
    assert tuner.blanker_stats() == want.stats
    # a caller's device tensor is left as it is, unless in_place
    xd = t.from_numpy(x.copy()).cuda()
    tuner.load(xd)
    assert _spectrum(hip, tuner, N).tobytes() == ref.tobytes() and xd.cpu().numpy().tobytes() == x.tobytes()
    tuner.set_blanker(nb, in_place=True)
    tuner.load(xd)
    assert _spectrum(hip, tuner, N).tobytes() == ref.tobytes() and xd.cpu().numpy().tobytes() == want.out.tobytes()
    assert tuner.blanker_stats() == want.stats
    # off again: the bits of a tuner that never had one
    tuner.set_blanker(None)
    tuner.load(x)
    assert _spectrum(hip, tuner, N).tobytes() == never.tobytes()
    # raw formats
    for k, fmt in ((1, "cs16"), (2, "cu8")):
        xr, wr = _model(fmt, N, 400 + k)
        plain.load_raw(wr.out)
        ref = _spectrum(hip, plain, N)
        plain.load_raw(nb.run(xr))
        assert _spectrum(hip, plain, N).tobytes() == ref.tobytes()
        tuner.set_blanker(nb)
        tuner.load_raw(xr)
        assert _spectrum(hip, tuner, N).tobytes() == ref.tobytes() and tuner.blanker_stats() == wr.stats
        xd = t.from_numpy(xr.copy()).cuda()
        tuner.load_raw(xd)
        assert _spectrum(hip, tuner, N).tobytes() == ref.tobytes() and xd.cpu().numpy().tobytes() == xr.tobytes()


def test_lanes_follow_the_base_tuner_s_blanker(rc, hip):
    N = TUNER_SIZES[0]
    nb = _blanker(rc)
    xs = [_model("cf32", N, 410 + k) for k in range(3)]
    single = _tuner(rc, N)
    single.set_blanker(nb)
    want = []
    for x, model in xs:
        single.load(x)
        want.append(single.run_all())
        assert single.blanker_stats() == model.stats
    clean = _tuner(rc, N)
    clean.load(xs[0][1].out)
    assert clean.run_all().tobytes() == want[0].tobytes()
    base = _tuner(rc, N)
    base.set_blanker(nb)
    lanes = rc.Lanes(base, depth=2)
    tickets = [lanes.submit(x) for x, _ in xs]
    for k, ticket in enumerate(tickets):
        assert lanes.result(ticket).tobytes() == want[k].tobytes()
    assert lanes._tuners[1]._blank_handles and lanes._tuners[1]._blank_handles is not base._blank_handles


def test_the_iq_balance_sees_the_blanked_buffer(rc, hip):
    N = TUNER_SIZES[0]
    nb = _blanker(rc)
    x, want = _model("cf32", N, 400)
    a, b = _tuner(rc, N), _tuner(rc, N)
    a.set_blanker(nb)
    a.set_iq_balance("auto", dc_notch=2)
    a.load(x)
    b.set_iq_balance("auto", dc_notch=2)
    b.load(want.out)
    assert _spectrum(hip, a, N).tobytes() == _spectrum(hip, b, N).tobytes()


def test_the_example_runs_and_the_blanker_helps_every_station(rc):
    spec = importlib.util.spec_from_file_location("airband_blanker", os.path.join(ROOT, "examples", "airband_blanker.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    on_air, before, after, stats, lifted0, lifted1, lift0, lift1 = ex.run(channels=40, rate=1_000_000, stations=5, pulses=40)
    for i, b, a in zip(on_air, before, after):
        print("channel %2d: audio error %.4f without the blanker, %.4f with it" % (i, b, a))
        assert a < b
    print("stats", stats, "empty channels over the threshold:", lifted0, "->", lifted1, "lift %.1f -> %.1f dB" % (lift0, lift1))
    assert stats[0] == 40 * ex.PULSE and stats[1] >= stats[0] and lifted1 <= lifted0 and lift1 < lift0
