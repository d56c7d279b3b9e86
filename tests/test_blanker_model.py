"""CPU: the noise blanker's numpy model (tests/blanker_model.py) against a sample-by-sample restatement of the definition
(include/rcfm.h, "noise blanker"), the integer rounding and the CU8 centre, the robustness of every input the GPU test
(tests/test_hip_blanker.py) compares exactly, and what the blanker buys on the example's buffer."""

import importlib.util
import os

import numpy as np
import pytest

import blanker_model as bm
from conftest import ROOT

f32 = np.float32


def _tree(v):
    return v[0] if len(v) == 1 else _tree(v[:len(v) // 2]) + _tree(v[len(v) // 2:])


def brute(x, block, span, mode, value, hold, ramp):
    """The definition, one sample at a time, O(n G): (t, hit, d capped at G + 1, g, out)."""
    re, im = bm.components(x)
    n = re.shape[0]
    nb = -(-n // block)
    ramp = [f32(v) for v in ramp]
    G = hold + len(ramp)
    p = [f32(f32(re[i] * re[i]) + f32(im[i] * im[i])) for i in range(n)]
    m = []
    for b in range(nb):
        slots = [float(re[i]) ** 2 + float(im[i]) ** 2 if i < n else 0.0 for i in range(b * block, (b + 1) * block)]
        v = _tree(slots) / float(min(block, n - b * block))
        m.append(v if np.isfinite(v) else np.inf)
    t = []
    for b in range(nb):
        w = sorted(m[max(0, b - span):min(nb - 1, b + span) + 1])
        t.append(f32(value) if mode == bm.ABSOLUTE else f32(np.float64(value) * w[(len(w) - 1) // 2]))
    hit = [bool(p[i] > t[i // block]) for i in range(n)]
    d, g = [], []
    for i in range(n):
        near = [abs(i - j) for j in range(max(0, i - G), min(n, i + G + 1)) if hit[j]]
        di = min(near) if near else G + 1
        d.append(di)
        g.append(f32(0) if di <= hold else ramp[di - hold - 1] if di <= G else f32(1))
    xs = np.asarray(x)
    out = xs.copy().reshape(-1) if xs.dtype == np.complex64 else xs.copy().reshape(-1, 2)
    for i in range(n):
        if g[i] == 1:
            continue
        if xs.dtype == np.complex64:
            out[i] = 0 if g[i] == 0 else complex(f32(g[i] * re[i]), f32(g[i] * im[i]))
        elif xs.dtype == np.uint8:
            for c in range(2):
                u = f32(xs.reshape(-1, 2)[i, c])
                out[i, c] = 127 + (i & 1) if g[i] == 0 else int(np.rint(f32(f32(127.5) + f32(g[i] * f32(u - f32(127.5))))))
        else:
            for c in range(2):
                out[i, c] = 0 if g[i] == 0 else int(np.rint(f32(g[i] * f32(xs.reshape(-1, 2)[i, c]))))
    return np.array(t, f32), np.array(hit), np.array(d), np.array(g, f32), out.reshape(xs.shape)


TINY = [(fmt, n, 64, span, hold, R, mode, 50 + k)
        for k, (fmt, n, span, hold, R, mode) in enumerate([
            ("cf32", 1, 0, 0, 0, bm.MEDIAN), ("cs16", 1, 1, 0, 5, bm.MEDIAN), ("cu8", 3, 0, 2, 3, bm.MEDIAN), ("cs16", 63, 1, 0, 5, bm.MEDIAN), ("cs8", 64, 0, 2, 3, bm.ABSOLUTE),
            ("cu8", 65, 1, 1, 4, bm.MEDIAN), ("cf32", 200, 8, 3, 0, bm.MEDIAN), ("cs16", 257, 0, 0, 0, bm.ABSOLUTE),
            ("cu8", 300, 4, 8, 8, bm.ABSOLUTE), ("cs8", 321, 1, 40, 30, bm.MEDIAN), ("cf32", 130, 1, 0, 9, bm.ABSOLUTE)])]


@pytest.mark.parametrize("case", TINY, ids=lambda c: "%s-n%d-W%d-H%d-R%d-m%d" % (c[0], c[1], c[3], c[4], c[5], c[6]))
def test_model_equals_the_sample_by_sample_definition(case):
    x, kw = bm.case_input(case)
    if case[1] == 130:                                  # a ramp that is not monotonic, and holds a 1 and a 0: used as given
        kw["ramp"] = np.array([0.5, 0.25, 1.0, 0.0, 0.75, 0.125, 0.9, 0.3, 0.6], f32)
    got = bm.blank(x, **kw)
    t, hit, d, g, out = brute(x, **kw)
    G = kw["hold"] + len(kw["ramp"])
    assert np.array_equal(got.t.view(np.uint32), t.view(np.uint32))
    assert np.array_equal(got.hit, hit) and (hit.any() or case[1] <= 3)
    if not hit.any():
        assert np.all(got.g == 1) and got.out.tobytes() == np.ascontiguousarray(x).tobytes()
    assert np.array_equal(np.minimum(got.d, G + 1), d)
    assert np.array_equal(got.g.view(np.uint32), g.view(np.uint32))
    assert got.out.dtype == out.dtype and got.out.tobytes() == out.tobytes()
    assert got.stats == (int(hit.sum()), int((g < 1).sum()))
    assert np.array_equal(bm.mask_words(got.hit)[:-(-case[1] // 32)],
                          [sum(int(hit[i]) << (i - 32 * w) for i in range(32 * w, min(32 * w + 32, case[1])))
                           for w in range(-(-case[1] // 32))])


def test_lower_median_and_short_last_block():
    """nb < 2 W + 1, an even count, and the last block's mean over its own samples only."""
    re = np.concatenate([np.full(64, 1.0), np.full(64, 3.0), np.full(64, 2.0), np.full(10, 4.0)]).astype(f32)
    m = bm.block_means(re, np.zeros_like(re), 64)
    assert np.array_equal(m, [1.0, 9.0, 4.0, 16.0])
    assert np.array_equal(bm.thresholds(m, 0, bm.MEDIAN, 2.0), f32([2, 18, 8, 32]))
    assert np.array_equal(bm.thresholds(m, 1, bm.MEDIAN, 1.0), f32([1, 4, 9, 4]))       # (1 9) (1 4 9) (4 9 16) (4 16)
    assert np.array_equal(bm.thresholds(m, 8, bm.MEDIAN, 1.0), f32([4, 4, 4, 4]))       # element 1 of (1 4 9 16)
    assert np.array_equal(bm.thresholds(m, 8, bm.ABSOLUTE, 0.1), np.full(4, f32(0.1)))
    bad = bm.block_means(np.array([np.nan] + [1.0] * 63 + [np.inf] + [1.0] * 63, f32), np.zeros(128, f32), 64)
    assert np.all(np.isposinf(bad))


def test_integer_rounding_and_the_cu8_centre():
    g = np.array([0.5, 0.5, 0.5, 0.5, 0.0, 0.0, 1.0, 0.25], f32)
    cs16 = np.array([[-32768, 32767], [1, 3], [-1, -3], [5, -5], [-32768, 7], [9, 9], [-32768, 32767], [2, 6]], np.int16)
    assert bm.output(cs16, g).tolist() == [[-16384, 16384], [0, 2], [0, -2], [2, -2], [0, 0], [0, 0], [-32768, 32767], [0, 2]]
    cs8 = np.array([[-128, 127], [1, 3], [-1, -3], [5, -5], [-128, 7], [9, 9], [-128, 127], [2, 6]], np.int8)
    assert bm.output(cs8, g).tolist() == [[-64, 64], [0, 2], [0, -2], [2, -2], [0, 0], [0, 0], [-128, 127], [0, 2]]
    cu8 = np.array([[255, 0], [128, 127], [130, 125], [129, 126], [255, 0], [3, 200], [255, 0], [0, 255]], np.uint8)
    # 127.5 + g (u - 127.5): 191.25 63.75 | 127.75 127.25 | 128.75 126.25 | 128.25 126.75 | centre | centre | copy | 95.625 159.375
    assert bm.output(cu8, g).tolist() == [[191, 64], [128, 127], [129, 126], [128, 127], [127, 127], [128, 128], [255, 0], [96, 159]]
    # the zero of CU8 alternates with the sample's index, whatever the sample held: no DC step against a centre of 127.5
    z = bm.output(np.full((6, 2), 200, np.uint8), np.zeros(6, f32))
    assert z.tolist() == [[127, 127], [128, 128]] * 3 and float(z.mean()) == 127.5
    # complex64: bit copies where g = 1 (a NaN payload and -0 survive), +0 where g = 0
    c = np.array([0x7fc12345, 0x80000000, 0x3f800000, 0xbf800000, 0x7f800000, 0x80000000], np.uint32).view(np.complex64)
    out = bm.output(c, np.array([1.0, 0.5, 0.0], f32)).view(np.uint32)
    assert out.tolist() == [0x7fc12345, 0x80000000, 0x3f000000, 0xbf000000, 0, 0]


def all_inputs():
    from test_hip_blanker import exact_inputs
    return exact_inputs()


def test_every_input_of_the_gpu_test_is_robust():
    """No sample's power lies within 2^-22 of its threshold: the one tolerance of the GPU test, a threshold one float32 ulp
    from the model's, cannot change a hit."""
    count = 0
    for name, x, kw in all_inputs():
        assert bm.robust(x, **kw), name
        count += 1
    assert count > 120
    # ... and `robust` does see a sample that sits on its threshold
    x = bm.make_input("cf32", 256, 7)
    t = bm.blank(x, block=64, span=1).t
    x[100] = np.sqrt(np.float64(t[1])) * (1 + 2.0 ** -24)
    assert not bm.robust(x, block=64, span=1)


def test_the_blanker_lowers_every_station_s_envelope_error_on_the_example_s_buffer():
    """examples/airband_blanker.py's buffer at a size a CPU test can take (40 channels at 1 MS/s, 5 stations, 40 pulses): per
    station on the air, the envelope error against the pulse-free buffer is smaller after blanking than before."""
    spec = importlib.util.spec_from_file_location("airband_blanker", os.path.join(ROOT, "examples", "airband_blanker.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    clean, dirty, centres, f_in, on_air = ex.buffers(channels=40, rate=1_000_000, stations=5, pulses=40)
    n = dirty.shape[0]
    kw = dict(block=4096, span=4, mode=bm.MEDIAN, value=10.0 ** 1.2, hold=int(round(2e-6 * n)),
              ramp=bm.raised_cosine(int(round(1e-6 * n))))
    res = bm.blank(dirty, **kw)
    assert bm.blank(clean, **kw).stats == (0, 0)                       # no false hit on the clean buffer
    assert res.stats[0] == 40 * ex.PULSE
    before = ex.envelope_errors(dirty, clean, centres, f_in, on_air)
    after = ex.envelope_errors(res.out, clean, centres, f_in, on_air)
    for i, b, a in zip(on_air, before, after):
        print("channel %2d: envelope error %.4f before, %.4f after" % (i, b, a))
        assert a < b, (i, b, a)
    print("hits %d, blanked %d of %d samples (%.3f %%)" % (res.stats + (n, 100.0 * res.stats[1] / n)))
