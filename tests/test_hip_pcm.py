"""GPU: rcfm_audio_pack and Tuner.run_all_packed against tests/pcm_model.py -- bit for bit, no tolerance.

Every call gets its buffers pre-filled with sentinels: rows >= n_open of `packed`, entries >= n_open of `index` and the
guard elements around both must come back untouched.  Closed rows of the input are NaN (a closed row that was read and
stored anywhere would show), open rows are noise at 0.5 RMS with NaN, +-inf, +-1, exact rounding ties and values just
beyond full scale planted in them.  Natural alignment is an argument requirement (RCFM_ERR_ARG otherwise), so the
misaligned cases offset `audio` by one float and `packed` by one element of its format: 2 bytes for int16, 4 for float32;
both leave the 16-byte vector path.
"""

import ctypes

import numpy as np
import pytest

import pcm_model
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

S16, F32 = pcm_model.S16, pcm_model.F32
FORMATS = [pytest.param(S16, id="s16"), pytest.param(F32, id="f32")]
GUARD = 8                    # sentinel elements in front of and behind every output
SENT16, SENT32, SENT_INDEX, SENT_N = 0x5A5A, 0x5A5A5A5A, -7, -9


@pytest.fixture(scope="module")
def hip():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    from radiocore._internal import hip
    return hip


def _segment():
    from radiocore._internal import hip
    return hip.RCFM_PACK_SEGMENT


ROWS = sorted({1, 3, 7, 8, 9, 250, 4096, 4097, 4104, 8000, 96000, _segment() - 1, _segment() + 1})
COUNTS = [(1, 8), (2, 8), (255, 8), (256, 8), (257, 8), (1025, 8), (8192, 8), (65535, 2)]
MASKS = {
    "all_open": lambda n: np.ones(n, np.uint8),
    "all_closed": lambda n: np.zeros(n, np.uint8),
    "alternating": lambda n: (np.arange(n) % 2).astype(np.uint8),
    "first_only": lambda n: (np.arange(n) == 0).astype(np.uint8),
    "last_only": lambda n: (np.arange(n) == n - 1).astype(np.uint8),
    "bytes_255": lambda n: np.where(np.arange(n) % 3 == 1, 255, 0).astype(np.uint8),
    "seeded_10_percent": lambda n: (np.random.default_rng(n).random(n) < 0.1).astype(np.uint8),
    "null": lambda n: None,
}


def _audio(count, row, mask, gain, seed):
    """float32 [count, row]: see the module docstring."""
    rng = np.random.default_rng(seed)
    a = (0.5 * rng.standard_normal((count, row))).astype(np.float32)
    is_open = np.ones(count, bool) if mask is None else mask != 0
    k = np.array([0, 1, 2, 3, 100, 32765, 32766, -1, -2, -3, -32766, -32767], np.float64)
    special = np.concatenate([
        np.array([0x7fc00001, 0xffc12345, 0x7f800001], np.uint32).view(np.float32),       # NaNs with payloads
        np.array([np.inf, -np.inf, 1.0, -1.0, 1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20, 3e38, -3e38, 0.0, -0.0], np.float32),
        np.array([1, 0x807fffff], np.uint32).view(np.float32),                             # denormals
        ((k + 0.5) / gain).astype(np.float32),                                             # ties (exact when gain is 2^k)
        (np.float32(32767.4) / np.float32(gain), np.float32(-32767.6) / np.float32(gain))])
    rows = np.flatnonzero(is_open)
    if rows.size:
        cells = rows.size * row
        pos = rng.choice(cells, size=min(special.size, cells), replace=False)
        bits = a.view(np.uint32)
        bits[rows[pos // row], pos % row] = special.view(np.uint32)[:pos.size]
    a.view(np.uint32)[~is_open] = 0x7fc00bad                                               # closed rows: NaN
    return a


def _pack(hip, audio, mask, fmt, gain, audio_off=0, packed_off=0, stream=None, want_index=True):
    """One rcfm_audio_pack of the numpy input on the device; (index [count], packed [count, row], n_open) as numpy, after
    the guards were checked.  audio_off / packed_off: elements the buffers start off their 256-byte aligned allocation."""
    import torch
    lib = hip.lib()
    count, row = audio.shape
    a_dev = torch.zeros(audio_off + count * row, dtype=torch.int32, device="cuda")
    a_dev[audio_off:] = torch.from_numpy(audio.reshape(-1).view(np.int32)).cuda()
    o_dev = None if mask is None else torch.from_numpy(mask).cuda()
    el, sent, tdt = (2, SENT16, torch.int16) if fmt == S16 else (4, SENT32, torch.int32)
    p_dev = torch.full((GUARD + packed_off + count * row + GUARD,), sent, dtype=tdt, device="cuda")
    i_dev = torch.full((GUARD + count + GUARD,), SENT_INDEX, dtype=torch.int32, device="cuda")
    n_dev = torch.full((3,), SENT_N, dtype=torch.int32, device="cuda")
    s = hip.stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    hip.check(lib.rcfm_audio_pack(ctypes.c_void_p(a_dev.data_ptr() + 4 * audio_off), None if o_dev is None else hip.ptr(o_dev),
                                  count, row, fmt, gain, ctypes.c_void_p(p_dev.data_ptr() + el * (GUARD + packed_off)),
                                  ctypes.c_void_p(i_dev.data_ptr() + 4 * GUARD) if want_index else None,
                                  ctypes.c_void_p(n_dev.data_ptr() + 4) if want_index else None, s))
    if stream is not None:
        stream.synchronize()
    p, ix, n = p_dev.cpu().numpy(), i_dev.cpu().numpy(), n_dev.cpu().numpy()
    lo = GUARD + packed_off
    assert np.all(p[:lo] == p.dtype.type(sent)) and np.all(p[lo + count * row:] == p.dtype.type(sent)), "a guard of packed was written"
    assert np.all(ix[:GUARD] == SENT_INDEX) and np.all(ix[GUARD + count:] == SENT_INDEX), "a guard of index was written"
    assert n[0] == SENT_N and n[2] == SENT_N
    return ix[GUARD:GUARD + count], p[lo:lo + count * row].reshape(count, row), int(n[1])


def _check(got, audio, mask, fmt, gain, what):
    index, packed, n_open = got
    count = audio.shape[0]
    want_index, want_rows, want_n = pcm_model.pack(audio, mask, fmt, gain)
    assert n_open == want_n, (what, n_open, want_n)
    assert np.array_equal(index[:want_n], want_index), what
    assert np.all(index[want_n:] == SENT_INDEX), (what, "index written beyond n_open")
    sent = SENT16 if fmt == S16 else SENT32
    assert np.array_equal(pcm_model.bits(packed[:want_n]), pcm_model.bits(want_rows).reshape(want_n, packed.shape[1])), what
    assert np.all(pcm_model.bits(packed[want_n:count]) == sent), (what, "rows written beyond n_open")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("row", ROWS)
def test_rows(hip, row, fmt):
    """Every row length of the issue's list and one on each side of the kernel's segment (hip.RCFM_PACK_SEGMENT); five
    channels, three open (one of them by a byte of 255).  gain = 32768: the planted ties are exact."""
    mask = np.array([255, 0, 1, 1, 0], np.uint8)
    audio = _audio(5, row, mask, 32768.0, seed=row)
    _check(_pack(hip, audio, mask, fmt, 32768.0), audio, mask, fmt, 32768.0, ("row", row))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("count,row", COUNTS)
def test_counts(hip, count, row, fmt):
    """The scan across its thread, wave and workgroup-size boundaries, a seeded 10 % mask; the default gain."""
    mask = MASKS["seeded_10_percent"](count)
    audio = _audio(count, row, mask, 32767.0, seed=count)
    _check(_pack(hip, audio, mask, fmt, 32767.0), audio, mask, fmt, 32767.0, ("count", count))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", sorted(MASKS))
def test_masks(hip, name, fmt):
    """Every mask of the CPU list, a seeded 10 % one and open = NULL, at a count that is no multiple of anything (257) and
    at five channels of a row with a partial last segment."""
    for count, row in ((257, 8), (5, 4104)):
        mask = MASKS[name](count)
        audio = _audio(count, row, mask, 32768.0, seed=count + row)
        _check(_pack(hip, audio, mask, fmt, 32768.0), audio, mask, fmt, 32768.0, (name, count, row))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("row", [8, 250, 4096, 8000])
def test_misaligned_pointers_take_the_element_path(hip, row, fmt):
    """audio 4 bytes off, packed one element off (2 bytes for int16, 4 for float32), each alone and both together."""
    mask = np.array([1, 1, 0, 255], np.uint8)
    audio = _audio(4, row, mask, 32768.0, seed=row + 1)
    for a_off, p_off in ((1, 0), (0, 1), (1, 1)):
        _check(_pack(hip, audio, mask, fmt, 32768.0, audio_off=a_off, packed_off=p_off), audio, mask, fmt, 32768.0,
               ("misaligned", row, a_off, p_off))


def test_index_and_n_open_may_be_null(hip):
    mask = MASKS["alternating"](9)
    audio = _audio(9, 24, mask, 32767.0, seed=4)
    index, packed, n = _pack(hip, audio, mask, S16, 32767.0, want_index=False)
    assert n == SENT_N and np.all(index == SENT_INDEX)
    _, want, k = pcm_model.pack(audio, mask, S16, 32767.0)
    assert np.array_equal(packed[:k], want) and np.all(packed[k:] == SENT16)


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_streams_and_two_runs_give_identical_bits(hip, fmt):
    import torch
    count, row = 1025, 4104
    mask = MASKS["seeded_10_percent"](count)
    audio = _audio(count, row, mask, 32767.0, seed=77)
    streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]
    runs = [_pack(hip, audio, mask, fmt, 32767.0, stream=s) for s in streams + streams[1:]]
    _check(runs[0], audio, mask, fmt, 32767.0, "default stream")
    for r in runs[1:]:
        assert r[2] == runs[0][2] and np.array_equal(r[0], runs[0][0])
        assert np.array_equal(pcm_model.bits(r[1]), pcm_model.bits(runs[0][1]))


# ---- Tuner.run_all_packed ------------------------------------------------------------------------------------------------

def _tuner_pair(kind):
    """(plain tuner, packing tuner on cuda=True, buffer): two tuners of one geometry run in lockstep, so that the
    de-emphasis state of WBFM is the same in both whatever ran before."""
    import radiocore as rc
    import am_model
    import squelch_model
    import workloads
    if kind == "AM":
        N, B, A, C = 200_000, 25_000, 8_000, 8
        centres = workloads.channel_grid(C, B)
    else:
        N, B, A = 600_000, 60_000, 12_000
        centres = [100.00e6, 100.05e6, 99.90e6]
    tuners = []
    for cuda in (False, True):
        t = rc.Tuner(cuda=cuda)
        for f in centres:
            t.add_channel(f, B, getattr(rc, kind)(B, A, cuda=cuda))
        t.request_bandwidth(float(N))
        tuners.append(t)
    if kind == "AM":
        x = squelch_model.sparse_band(N, tuners[0].input_frequency, centres, B,
                                      {i: am_model.station(i, B, seed=5) for i in (1, 4, 6)}, seed=3)
    else:
        x = workloads.wideband(N, tuners[0].input_frequency, centres, B, gain=0.5)
    return tuners[0], tuners[1], x


@pytest.mark.parametrize("kind,n_stations", [("AM", 3), ("WBFM", 2)])
def test_run_all_packed(hip, kind, n_stations):
    """A small AM tuner (N = 200 000, eight 25 kHz channels -> 8 kHz, three stations) and the three-channel WBFM one of
    smoke() (ch = 2): run_all_packed equals pcm_model.pack of run_all's audio and open_mask(), with squelch on and off,
    numpy and device output, both formats."""
    import radiocore as rc
    plain, packing, x = _tuner_pair(kind)
    C = len(plain.channels())
    plain.load(x)
    packing.load(x)
    lv = plain.levels()
    threshold = float(np.sort(lv)[-n_stations])          # the n strongest channels are open (levels are bit-reproducible)
    for squelch in (None, threshold):
        plain.set_squelch(squelch)
        packing.set_squelch(squelch)
        for pcm in (rc.PCM(), rc.PCM("int16", 8192.0), rc.PCM("float32")):
            for device in (False, True):
                base = plain.run_all()
                mask = plain.open_mask().astype(np.uint8) if squelch is not None else None
                want_index, want_rows, want_n = pcm_model.pack(base, mask, pcm.format, pcm.gain)
                assert want_n == (n_stations if squelch is not None else C)
                got = packing.run_all_packed(pcm, numpy_output=not device)
                what = (kind, squelch, pcm, device)
                if device:
                    index, packed, n_open = got
                    assert index.is_cuda and packed.is_cuda and n_open.is_cuda
                    assert tuple(packed.shape) == base.shape and tuple(index.shape) == (C,) and tuple(n_open.shape) == (1,)
                    n = int(n_open.cpu()[0])
                    index, packed = index.cpu().numpy()[:n], packed.cpu().numpy()[:n]
                else:
                    index, packed = got
                    n = index.shape[0]
                assert n == want_n and index.dtype == np.int32 and np.array_equal(index, want_index), what
                assert packed.dtype == pcm.dtype and packed.shape == want_rows.shape, what
                assert np.array_equal(pcm_model.bits(packed), pcm_model.bits(want_rows)), what
                if squelch is not None:
                    assert np.array_equal(packing.open_mask(), plain.open_mask())
                else:
                    with pytest.raises(RuntimeError):
                        packing.open_mask()
    assert np.abs(want_rows).max() > 0
