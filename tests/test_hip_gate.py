"""GPU: the frame gate (include/rcfm.h, "frame gate") against tests/gate_model.py.

rcfm_frame_power: within 1 float32 ulp of the float64 sum over the same float32 input -- the products are exact in
float64, the sums are float64, there is one rounding -- and bit-identical from run to run, between streams, for a sub-range
of rows and for rows on 4- and 8-byte boundaries.
rcfm_tuner_frame_levels: bit-identical to rcfm_tuner_run + rcfm_frame_power chunked the same way; the mean over a channel's
frames against rcfm_tuner_levels within 2e-5 relative on stations within 20 dB of the strongest (tests/test_hip_squelch.py
asserts 5e-6 for the levels, tests/test_hip_tuner_gather.py bounds the whole path's amplitude by 2.8e-6: 5e-6 + 2 x 2.8e-6,
rounded up).
rcfm_gate_run / rcfm_gate_apply: masks, states and output bits equal the model's.
Through the Tuner: masks equal the model's for buffers whose model frame powers tests/test_gate_model.py proves to lie
>= 3 dB from every threshold; the audio equals the model's apply of the same run without a gate, bit for bit.
"""

import ctypes

import numpy as np
import pytest

import gate_model as gm
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

REL_LEVELS = 2e-5


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
def torch(rc):
    import torch
    return torch


def _dev(torch, a, offset_floats=0):
    """The array on the device, its first element `offset_floats` floats behind an allocation's start."""
    a = np.ascontiguousarray(a)
    flat = torch.from_numpy(a.view(np.uint8).reshape(-1))
    buf = torch.empty(flat.numel() + 4 * offset_floats + 64, dtype=torch.uint8, device="cuda")
    view = buf[4 * offset_floats:4 * offset_floats + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 256 == (4 * offset_floats) % 256
    return view


def _host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def _stream_ptr(s):
    return ctypes.c_void_p(s.cuda_stream)


# ---- rcfm_frame_power ----------------------------------------------------------------------------------------------------

def _frame_power(hip, torch, xd, rows, n, is_complex, L, stream=None):
    F = n // L
    out = torch.full((rows * F + 1,), -1.0, dtype=torch.float32, device="cuda")
    hip.check(hip.lib().rcfm_frame_power(ctypes.c_void_p(xd.data_ptr()), rows, n, is_complex, L, hip.ptr(out),
                                         hip.stream() if stream is None else _stream_ptr(stream)))
    if stream is not None:
        stream.synchronize()
    got = out.cpu().numpy()
    assert got[-1] == -1.0                       # nothing behind the last frame was written
    return got[:-1].reshape(rows, F)


LENGTHS = [1, 2, 3, 63, 64, 65, 250, 1000, 8193, 20001]


@pytest.mark.parametrize("is_complex", [0, 1])
def test_frame_power_against_float64(hip, torch, is_complex):
    """Every L, n with and without a tail, odd n, 1 .. 5 rows three decades apart in level.  L = 1000 complex is a wave's
    frame of 2000 floats, L = 8193 a workgroup's, L = 8193 complex and 20 001 two and three segments."""
    rng = np.random.default_rng(7 + is_complex)
    worst = 0.0
    for k, L in enumerate(LENGTHS):
        for tail in sorted({0, min(L - 1, 4), min(L - 1, 5)}):     # none, and a tail that makes n odd (L > 1)
            n = 3 * L + tail
            if tail and n % 2 == 0:
                continue
            rows = 1 + (k + tail) % 5
            scale = 10.0 ** (-3.0 * np.arange(rows) / max(rows - 1, 1))[:, None]
            x = rng.standard_normal((rows, n)) * scale
            if is_complex:
                x = x + 1j * rng.standard_normal((rows, n)) * scale
            x = x.astype(np.complex64 if is_complex else np.float32)
            got = _frame_power(hip, torch, _dev(torch, x), rows, n, is_complex, L)
            ref = gm.frame_power(x, L)
            assert got.shape == ref.shape == (rows, n // L) and got.dtype == np.float32
            ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
            err = float(np.max(np.abs(got.astype(np.float64) - ref) / ulp))
            worst = max(worst, err)
            assert err <= 1.0, (L, n, rows, err)
    print("frame power, complex=%d: worst error %.3f ulp" % (is_complex, worst))


@pytest.mark.parametrize("is_complex,L,n", [(0, 250, 1001), (1, 250, 1001), (0, 8193, 24583), (1, 20001, 60005), (1, 65, 197)])
def test_frame_power_bit_identity(hip, torch, is_complex, L, n):
    """Two runs; a second stream; rows 1 - 2 alone against rows 1 - 2 of three; a base 4 (real) or 8 (complex) but not 16
    bytes aligned -- and with odd n the rows themselves start on such boundaries."""
    rng = np.random.default_rng(L)
    rows, comp = 3, 2 if is_complex else 1
    x = rng.standard_normal((rows, n * comp)).astype(np.float32)
    xd = _dev(torch, x)
    first = _frame_power(hip, torch, xd, rows, n, is_complex, L)
    assert np.array_equal(first, _frame_power(hip, torch, xd, rows, n, is_complex, L))
    torch.cuda.synchronize()
    assert np.array_equal(first, _frame_power(hip, torch, xd, rows, n, is_complex, L, stream=torch.cuda.Stream()))
    sub = _frame_power(hip, torch, xd[4 * n * comp:], 2, n, is_complex, L)
    assert np.array_equal(first[1:], sub)
    shifted = _dev(torch, x, offset_floats=comp)
    assert shifted.data_ptr() % 16 == 4 * comp
    assert np.array_equal(first, _frame_power(hip, torch, shifted, rows, n, is_complex, L))


# ---- rcfm_tuner_frame_levels ---------------------------------------------------------------------------------------------

def test_tuner_frame_levels(rc, hip, torch):
    lib = hip.lib()
    N, B, C = 40000, 2000, 5
    chans = [(100.0e6 + B * (c - 2), B) for c in range(C)]
    tuner = rc.Tuner()
    for f, bw in chans:
        tuner.add_channel(f, bw, None)
    tuner.request_bandwidth(float(N))
    rng = np.random.default_rng(11)
    t = np.arange(N, dtype=np.float64) / N
    x = 0.003 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    for c, (f, bw) in enumerate(chans):                  # 4 dB apart, each swept in level over the buffer
        x += 0.5 * 10.0 ** (-4.0 * c / 20.0) * (1.0 + 0.8 * np.cos(2 * np.pi * (3 + c) * t)) * \
            np.exp(2j * np.pi * (round(f - tuner.input_frequency) + 130 * (c - 2)) * t)
    tuner.load(x.astype(np.complex64))
    h = tuner._ready()
    s = hip.stream()
    scratch = torch.empty(C * B, dtype=torch.complex64, device="cuda")
    iq = torch.empty(C * B, dtype=torch.complex64, device="cuda")
    levels = torch.empty(C, dtype=torch.float32, device="cuda")
    hip.check(lib.rcfm_tuner_levels(h, 0, C, hip.ptr(levels), s))
    levels = levels.cpu().numpy().astype(np.float64)
    worst = 0.0
    for F in (1, 10, 16):
        L = B // F
        for m in (1, 2, 5):
            got = torch.full((C, F), -1.0, dtype=torch.float32, device="cuda")
            hip.check(lib.rcfm_tuner_frame_levels(h, 0, C, F, hip.ptr(scratch), ctypes.c_size_t(8 * B * m + 7), hip.ptr(got), s))
            want = torch.full((C, F), -2.0, dtype=torch.float32, device="cuda")
            for i in range(0, C, m):
                cnt = min(m, C - i)
                hip.check(lib.rcfm_tuner_run(h, i, cnt, hip.ptr(iq), s))
                hip.check(lib.rcfm_frame_power(hip.ptr(iq), cnt, B, 1, L, ctypes.c_void_p(want.data_ptr() + 4 * F * i), s))
            got, want = got.cpu().numpy(), want.cpu().numpy()
            assert np.array_equal(got, want), (F, m)
            rel = np.abs(got.astype(np.float64).mean(axis=1) - levels) / levels
            worst = max(worst, float(rel.max()))
            assert np.all(levels >= levels.max() * 1e-2) and rel.max() <= REL_LEVELS, (F, m, rel)
    print("frame levels: mean over frames against rcfm_tuner_levels, worst relative difference %.3g" % worst)
    assert np.array_equal(tuner.frame_levels(16), got)
    assert tuner.frame_levels(1).shape == (C, 1)
    # a sub-range through first; F must divide B; a scratch below one channel; readiness and range as rcfm_tuner_run
    part = torch.empty((2, 16), dtype=torch.float32, device="cuda")
    hip.check(lib.rcfm_tuner_frame_levels(h, 2, 2, 16, hip.ptr(scratch), ctypes.c_size_t(8 * B * 5), hip.ptr(part), s))
    assert np.array_equal(part.cpu().numpy(), got[2:4])
    args = (hip.ptr(scratch), ctypes.c_size_t(8 * B * 5), hip.ptr(part), s)
    for F in (32, 3, 2001):                                  # (16 divides 2000: 125 samples to a frame, the odd case above)
        assert lib.rcfm_tuner_frame_levels(h, 0, 2, F, *args) == -4
    assert lib.rcfm_tuner_frame_levels(h, 0, 2, 10, hip.ptr(scratch), ctypes.c_size_t(8 * B - 1), hip.ptr(part), s) == -4
    assert lib.rcfm_tuner_frame_levels(h, 4, 2, 10, *args) == -2
    hip.check(lib.rcfm_tuner_frame_levels(h, 1, 0, 10, *args))
    with pytest.raises(ValueError):
        tuner.frame_levels(32)
    fresh = rc.Tuner()
    for f, bw in chans:
        fresh.add_channel(f, bw, None)
    fresh.request_bandwidth(float(N))
    assert lib.rcfm_tuner_frame_levels(fresh._device_tuner(N), 0, 2, 10, *args) == -5          # before a load
    with pytest.raises(RuntimeError):
        fresh.frame_levels(10)


# ---- rcfm_gate_run -------------------------------------------------------------------------------------------------------

class _Gate:
    def __init__(self, hip, C, hang, lead, ramp):
        self.hip, self.lib, self.C = hip, hip.lib(), C
        h = ctypes.c_void_p()
        r = np.ascontiguousarray(ramp, dtype=np.float32)
        hip.check(self.lib.rcfm_gate_create(C, hang, lead, r.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if len(r) else None,
                                            len(r), ctypes.byref(h)))
        self.h = hip.Handle(h, self.lib.rcfm_gate_destroy)

    def state(self):
        s = np.full((self.C, 2), -7, np.int32)
        self.hip.check(self.lib.rcfm_gate_get_state(self.h.value, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.hip.stream()))
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, dtype=np.int32)
        self.hip.check(self.lib.rcfm_gate_set_state(self.h.value, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.hip.stream()))

    def run(self, torch, first, power, to, tc, want_any=True):
        count, F = power.shape
        pd, tod, tcd = (_dev(torch, np.asarray(a, np.float32)) for a in (power, to, tc))
        mask = torch.full((count * (F + 1) + 1,), 9, dtype=torch.uint8, device="cuda")
        any_ = torch.full((count + 1,), 9, dtype=torch.uint8, device="cuda")
        self.hip.check(self.lib.rcfm_gate_run(self.h.value, first, count, F, ctypes.c_void_p(pd.data_ptr()),
                                              ctypes.c_void_p(tod.data_ptr()), ctypes.c_void_p(tcd.data_ptr()), self.hip.ptr(mask),
                                              self.hip.ptr(any_) if want_any else None, self.hip.stream()))
        m, a = mask.cpu().numpy(), any_.cpu().numpy()
        assert m[-1] == 9 and a[-1] == 9 and (want_any or np.all(a == 9))
        return m[:-1].reshape(count, F + 1), a[:-1]


def _powers(rng, count, F):
    return rng.choice(np.array([0.1, 0.3, 0.5, 0.7, 1.0, 2.0, np.nan], dtype=np.float32), size=(count, F),
                      p=[0.25, 0.2, 0.1, 0.2, 0.1, 0.1, 0.05])


@pytest.mark.parametrize("hang,lead", [(0, 0), (3, 0), (0, 2), (3, 2), (3, 7), (0, 7)])
def test_gate_run_against_model(hip, torch, hang, lead):
    """Synthetic powers with values equal to a threshold and NaNs, NaN thresholds; two calls with the state carried; the
    second through a sub-range; more channels than one workgroup's threads."""
    rng = np.random.default_rng(10 * hang + lead)
    C, F = 300, 7
    gate = _Gate(hip, C, hang, lead, [])
    assert not gate.state().any()
    to = np.where(rng.random(C) < 0.1, np.nan, 1.0).astype(np.float32)
    tc = np.where(rng.random(C) < 0.05, np.nan, 0.5).astype(np.float32)
    p0, p1 = _powers(rng, C, F), _powers(rng, C, F)
    m, a = gate.run(torch, 0, p0, to, tc)
    wm, wa, ws = gm.gate_run(np.zeros((C, 2), np.int32), p0, to, tc, hang, lead)
    assert np.array_equal(m, wm) and np.array_equal(a, wa) and np.array_equal(gate.state(), ws)
    first, count = 37, 250
    m, a = gate.run(torch, first, p1[first:first + count], to[first:first + count], tc[first:first + count], want_any=False)
    wm, wa, ws1 = gm.gate_run(ws[first:first + count], p1[first:first + count], to[first:first + count],
                              tc[first:first + count], hang, lead)
    assert np.array_equal(m, wm)
    ws[first:first + count] = ws1
    assert np.array_equal(gate.state(), ws)                  # the channels outside the range kept theirs


def test_gate_state_round_trip_and_refusals(hip, torch):
    lib = hip.lib()
    gate = _Gate(hip, 5, 2, 1, gm.ramp(4))
    s = np.array([[1, 2], [0, 0], [1, 0], [0, 0], [1, 1]], np.int32)
    gate.set_state(s)
    assert np.array_equal(gate.state(), s)
    m, a = gate.run(torch, 0, np.full((5, 1), 0.1, np.float32), np.ones(5), np.full(5, 0.5))
    assert m.tolist() == [[1, 1], [0, 0], [1, 0], [0, 0], [1, 1]] and a.tolist() == [1, 0, 1, 0, 1]
    assert gate.state().tolist() == [[1, 1], [0, 0], [0, 0], [0, 0], [1, 0]]
    hip.check(lib.rcfm_gate_reset(gate.h.value, hip.stream()))
    assert not gate.state().any()
    for on in (1, 0):
        hip.check(lib.rcfm_gate_set_fence(gate.h.value, on))
        m, _ = gate.run(torch, 0, np.full((5, 2), 2.0, np.float32), np.ones(5), np.full(5, 0.5))
        assert m[:, 1:].all()
        hip.check(lib.rcfm_gate_reset(gate.h.value, hip.stream()))
    keep = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = hip.ptr(keep)
    assert lib.rcfm_gate_run(gate.h.value, 4, 2, 1, p, p, p, p, None, hip.stream()) == -2
    assert lib.rcfm_gate_run(gate.h.value, -1, 1, 1, p, p, p, p, None, hip.stream()) == -2
    hip.check(lib.rcfm_gate_run(gate.h.value, 5, 0, 1, p, p, p, p, None, hip.stream()))
    assert lib.rcfm_gate_apply(gate.h.value, p, 1, 4, 12, 1, p, hip.stream()) == -4          # R = 4 > A / F = 3
    hip.check(lib.rcfm_gate_apply(gate.h.value, p, 0, 4, 16, 1, p, hip.stream()))


# ---- rcfm_gate_apply -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("A,F,ch,R,offset", [(800, 10, 1, 0, 0), (800, 10, 1, 1, 0), (800, 10, 1, 80, 0), (800, 10, 1, 16, 1),
                                             (875, 7, 1, 5, 0), (960, 10, 2, 48, 0), (960, 10, 2, 47, 0), (960, 10, 2, 47, 2),
                                             (800, 1, 1, 16, 0), (6000, 1, 2, 3000, 0)])
def test_gate_apply_against_model(hip, torch, A, F, ch, R, offset):
    """Output bits equal the model's.  A = 875: rows on 4-byte boundaries and frames of 125 samples, the 4-byte form; R = 1
    and R = 47 of stereo end a ramp inside a lane's four floats; offset: the 16-byte form's shapes from a base it cannot
    use.  Every combination of g and gp in every row; a closed row holding NaN comes out +0.0, open samples keep their bits."""
    rng = np.random.default_rng(A + R)
    count = 9
    x = rng.standard_normal((count, A, ch)).astype(np.float32)
    mask = rng.integers(0, 2, (count, F + 1)).astype(np.uint8)
    mask[0], mask[1] = 0, 1
    x[0, ::3] = np.nan
    x[1, ::5] = np.nan
    x[1, 7] = np.float32(-0.0)
    if F > 1:
        mask[2, :4] = (0, 0, 1, 1)
        La = A // F
        x[2, :La] = np.nan                                   # closed behind closed
        x[2, 2 * La:3 * La] = np.nan                         # open behind open
    r = gm.ramp(R)
    gate = _Gate(hip, count, 0, 0, r)
    xd, md = _dev(torch, x, offset), _dev(torch, mask)
    hip.check(hip.lib().rcfm_gate_apply(gate.h.value, ctypes.c_void_p(md.data_ptr()), count, F, A, ch,
                                        ctypes.c_void_p(xd.data_ptr()), hip.stream()))
    got = _host(xd, np.float32, x.shape)
    want = gm.gate_apply(x, mask, r)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[0].view(np.uint32).any()
    assert np.array_equal(got[1].view(np.uint32), x[1].view(np.uint32))


# ---- through the Tuner ---------------------------------------------------------------------------------------------------

def _oracle_tuner(scene):
    import radiocore_oracle as oracle
    return scene.add_to(oracle.Tuner())


_SCENES = {}


def _scene(name):
    """(scene, buffers, the model's frame powers per buffer), computed once per scene and left unchanged."""
    if name not in _SCENES:
        scene = {"mixed": gm.mixed, "stereo": gm.stereo}.get(name, lambda: gm.narrow(name))()
        ref = _oracle_tuner(scene)
        xs = scene.buffers(ref.input_frequency)
        powers, worst = scene.powers(ref, xs)
        assert worst >= gm.MARGIN_DB                          # (asserted without a device by tests/test_gate_model.py)
        _SCENES[name] = (scene, xs, powers)
    return _SCENES[name]


def _gate(rc):
    return rc.FrameGate(frames=gm.FRAMES, hang=gm.HANG, lead=gm.LEAD, ramp=gm.RAMP)


def _tuner(rc, scene, demod, order=None):
    return scene.add_to(rc.Tuner(), demod, order)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _expect(plain, mask, A):
    return gm.gate_apply(plain, mask, gm.ramp(int(round(gm.RAMP * A))))


@pytest.mark.parametrize("kind", ["AM", "FM"])
def test_tuner_gate_three_buffers(rc, kind):
    """Stations keyed at frame boundaries, one across the buffer edge, one ending exactly at it: the masks equal the model's
    over three buffers (hang over the boundary, look-ahead), open-open frames are bit-identical to the run without a gate,
    closed frames are exact zeros, the fades are the model's products.  set_gate(None) restores the parent's bits."""
    scene, xs, powers = _scene(kind)
    A = 800
    demod = lambda B: getattr(rc, kind)(B, A)
    base, gated = _tuner(rc, scene, demod), _tuner(rc, scene, demod)
    to, tc = scene.thresholds()
    gated.set_gate(_gate(rc), open=to, close=tc)
    with pytest.raises(RuntimeError):
        gated.frame_mask()
    masks, anys = scene.masks(powers)
    plain = []
    for b, x in enumerate(xs):
        base.load(x)
        gated.load(x)
        plain.append(base.run_all())
        got = gated.run_all()
        assert np.array_equal(gated.frame_mask(), masks[b][:, 1:].astype(bool)), b
        assert np.array_equal(gated.open_mask(), anys[b].astype(bool)), b
        want = _expect(plain[b], masks[b], A)
        assert np.array_equal(_bits(got), _bits(want)), b
        F, La = gm.FRAMES, A // gm.FRAMES
        g, gp = masks[b][:, 1:] != 0, masks[b][:, :-1] != 0
        frames = got.reshape(scene.C, F, La)
        assert np.array_equal(_bits(frames[g & gp]), _bits(plain[b].reshape(scene.C, F, La)[g & gp]))
        assert not _bits(frames[~g & ~gp]).any()
        assert np.array_equal(gated.frame_levels(gm.FRAMES).shape, (scene.C, gm.FRAMES))
    assert any(m[:, 0].any() for m in masks[1:])                 # the state crossed a buffer edge
    gated.set_gate(None)
    gated.load(xs[-1])
    assert np.array_equal(_bits(gated.run_all()), _bits(plain[-1]))
    with pytest.raises(RuntimeError):
        gated.frame_mask()


def test_tuner_gate_next_to_squelch_raises(rc):
    scene, xs, powers = _scene("FM")
    t = _tuner(rc, scene, lambda B: rc.FM(B, 800))
    to, tc = scene.thresholds()
    t.set_squelch(1e-3)
    held = t._squelch
    with pytest.raises(ValueError):
        t.set_gate(_gate(rc), open=to, close=tc)
    assert t._gate is None and t._squelch is held
    t.set_squelch(None)
    t.set_gate(_gate(rc), open=to, close=tc)
    held = t._gate
    with pytest.raises(ValueError):
        t.set_squelch(1e-3)
    with pytest.raises(ValueError):
        t.set_gate(_gate(rc), open=tc, close=to)                 # close above open
    with pytest.raises(ValueError):
        t.set_gate(rc.FrameGate(frames=7), open=to)              # 7 divides neither 2000 nor 800
    assert t._gate is held and t._squelch is None


def test_tuner_gate_wbfm_stereo(rc):
    scene, xs, powers = _scene("stereo")
    A = 12000
    demod = lambda bw: rc.WBFM(bw, A)
    base, gated = _tuner(rc, scene, demod), _tuner(rc, scene, demod)
    to, tc = scene.thresholds()
    gated.set_gate(_gate(rc), open=to, close=tc)
    masks, anys = scene.masks(powers)
    for b, x in enumerate(xs):
        base.load(x)
        gated.load(x)
        plain, got = base.run_all(), gated.run_all()
        assert got.shape == (3, A, 2)
        assert np.array_equal(gated.frame_mask(), masks[b][:, 1:].astype(bool))
        assert np.array_equal(_bits(got), _bits(_expect(plain, masks[b], A)))


def test_tuner_gate_run_each_two_bandwidths(rc):
    scene, xs, powers = _scene("mixed")
    demod = lambda B: rc.FM(B, B * 2 // 5)                       # audio of 800 and 1600 samples
    base, gated = _tuner(rc, scene, demod), _tuner(rc, scene, demod)
    to, tc = scene.thresholds()
    gated.set_gate(_gate(rc), open=to, close=tc)
    masks, anys = scene.masks(powers)
    for b, x in enumerate(xs):
        base.load(x)
        gated.load(x)
        plain, got = base.run_each(), gated.run_each()
        assert np.array_equal(gated.frame_mask(), masks[b][:, 1:].astype(bool))
        assert np.array_equal(gated.open_mask(), anys[b].astype(bool))
        for c in range(scene.C):
            A = plain[c].shape[0]
            want = _expect(plain[c][None], masks[b][c:c + 1], A)[0]
            assert A == scene.chans[c][1] * 2 // 5 and np.array_equal(_bits(got[c]), _bits(want)), (b, c)
    assert sorted(gated._gate_handles) == [800, 1600]
    assert gated.frame_levels(gm.FRAMES).shape == (scene.C, gm.FRAMES)


def test_tuner_gate_packed_drain_and_tone_squelch(rc):
    """run_all_packed through a Drain publishes the channels with anything open -- the fade-out of the station that closed
    exactly at the buffer edge included; a tone squelch behind the gate closes what the gate left open."""
    from radiocore.tools import wire
    scene, xs, powers = _scene("FM")
    A = 800
    demod = lambda B: rc.FM(B, A)
    gated = _tuner(rc, scene, demod)
    to, tc = scene.thresholds()
    gated.set_gate(_gate(rc), open=to, close=tc)
    masks, anys = scene.masks(powers)
    pcm = rc.PCM("float32")
    drain = rc.Drain(scene.C, (A, 1), pcm.dtype, depth=2)
    base = _tuner(rc, scene, demod)
    for b, x in enumerate(xs[:2]):
        base.load(x)
        gated.load(x)
        want = _expect(base.run_all(), masks[b], A)
        gated.run_all_packed(pcm, drain=drain)
        with drain.next() as (index, rows):
            assert index.tolist() == np.flatnonzero(anys[b]).tolist()
            assert np.array_equal(_bits(np.asarray(rows)), _bits(want[index]))
    drain.close()
    assert anys[1][4] == 1 and not masks[1][4, 4:].any()         # published for its hang and fade-out alone
    # the tone squelch's verdict comes on top: no station carries the wanted tone, so everything closes
    gated.set_tones(rc.ToneBank([67.0], frame=400), want=0, ratio=0.9)
    gated.load(xs[2])
    audio = gated.run_all()
    assert np.array_equal(gated.frame_mask(), masks[2][:, 1:].astype(bool))
    assert not gated.open_mask().any() and not _bits(audio).any()
    assert wire.frames(gated.channels(), audio, gated.open_mask()) == []


def test_tuner_gate_lanes_growing_list_and_reset(rc):
    """Lanes(depth=2) is bit-identical to the loop, frame masks per ticket; the states follow a growing channel list;
    reset_states() closes every channel."""
    scene, xs, powers = _scene("FM")
    A = 800
    demod = lambda B: rc.FM(B, A)
    to, tc = scene.thresholds()
    masks, anys = scene.masks(powers)
    loop = _tuner(rc, scene, demod)
    loop.set_gate(_gate(rc), open=to, close=tc)
    want = []
    for x in xs:
        loop.load(x)
        want.append(loop.run_all())
    laned = _tuner(rc, scene, demod)
    laned.set_gate(_gate(rc), open=to, close=tc)
    lanes = rc.Lanes(laned, depth=2)
    tickets = [lanes.submit(x) for x in xs]
    for b, tk in enumerate(tickets):
        audio, omask, fmask = lanes.result(tk, open_mask=True, frame_mask=True)
        assert np.array_equal(_bits(audio), _bits(want[b])), b
        assert np.array_equal(fmask, masks[b][:, 1:].astype(bool)) and np.array_equal(omask, anys[b].astype(bool))
    # reset_states: the third buffer again, from closed channels
    loop.reset_states()
    loop.load(xs[2])
    loop.run_all()
    fresh, _ = scene.masks(powers[2:])
    assert np.array_equal(loop.frame_mask(), fresh[0][:, 1:].astype(bool)) and not fresh[0][:, 0].any()
    assert masks[2][0, 0] == 1 and np.array_equal(loop.open_mask(), fresh[0].any(axis=1))
    # a growing list: the outermost stations first (the input geometry is then final), the others join with buffer 1
    order = [0, 7, 1, 2, 3, 4, 5, 6]
    grow = rc.Tuner()
    gate = _gate(rc)
    for c in order[:2]:
        grow.add_channel(scene.chans[c][0], scene.chans[c][1], demod(scene.chans[c][1]))
    grow.request_bandwidth(float(scene.n))
    grow.set_gate(gate, open=to[order[:2]], close=tc[order[:2]])
    grow.load(xs[0])
    grow.run_all()
    assert np.array_equal(grow.frame_mask(), masks[0][order[:2], 1:].astype(bool))
    for c in order[2:]:
        grow.add_channel(scene.chans[c][0], scene.chans[c][1], demod(scene.chans[c][1]))
        grow.request_bandwidth(float(scene.n))
    grow.load(xs[1])
    with pytest.raises(ValueError):
        grow.run_all()                                           # two thresholds for eight channels
    grow.set_gate(gate, open=to[order], close=tc[order])
    late, _ = scene.masks(powers[1:], stations=order[2:])
    for b in (1, 2):
        grow.load(xs[b])
        grow.run_all()
        exp = np.concatenate([masks[b][order[:2]], late[b - 1]])
        assert np.array_equal(grow.frame_mask(), exp[:, 1:].astype(bool)), b
    assert masks[1][0, 0] == 1                                   # station 0 stayed open across the hand-over


def test_airband_gate_example():
    """examples/airband_gate.py at a reduced size: the gate loses nothing of any transmission and lets through no more than
    look-ahead, hang time and the two cut frames around each; the per-buffer squelch does worse on the same buffers."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("airband_gate", os.path.join(ROOT, "examples", "airband_gate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    totals, published, on_air = mod.run(channels=120, rate=4_000_000, stations=7)
    runs = sum(len(r) for r in on_air.values())
    assert len(on_air) == 7 and runs >= 7
    sent, lost, extra = totals["gate"]
    print("gate: %s, squelch: %s (published, lost, let through; samples of audio)" % (totals["gate"], totals["squelch"]))
    La = mod.AUDIO // mod.FRAMES
    assert lost == 0
    assert 0 < extra <= runs * (1 + 12 + 2) * La
    s_sent, s_lost, s_extra = totals["squelch"]
    assert s_lost + s_extra > lost + extra
    assert published and all(c in on_air and 0 <= a < b <= mod.AUDIO and a % La == 0 and b % La == 0 for _, c, a, b in published)
