"""GPU: radiocore.tools.Drain (rcfm_drain_*) -- packed audio through `depth` page-locked slots on two copy streams, against
the synchronous path and tests/pcm_model.py, bit for bit; the call-order refusals; examples/airband_pcm.py."""

import ctypes

import numpy as np
import pytest

import pcm_model
from conftest import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs an MI355X")]

ERR_STATE = -5
COUNT, SHAPE = 37, (250, 2)          # rows of 500 samples: 1000 bytes of int16, no multiple of 16
ROW = SHAPE[0] * SHAPE[1]


@pytest.fixture(scope="module")
def hip():
    import radiocore
    assert radiocore.HasCuda(), "librcfm.so did not load or sees no device"
    from radiocore._internal import hip
    return hip


def _buffers(masks, seed=0):
    rng = np.random.default_rng(seed)
    return [(0.5 * rng.standard_normal((COUNT,) + SHAPE)).astype(np.float32) for _ in masks]


def _submit(hip, drain, audio, mask, fmt, gain):
    """rcfm_audio_pack of one buffer into the drain's next slot, then submit: what Tuner.run_all_packed(drain=) does.
    Returns the device tensors, to be kept until the buffer has been handed out."""
    import torch
    a = torch.from_numpy(audio).cuda()
    m = torch.from_numpy(mask).cuda()
    packed, index, n_open = drain._begin()
    hip.check(hip.lib().rcfm_audio_pack(hip.ptr(a), hip.ptr(m), COUNT, ROW, fmt, gain, packed, index, n_open, hip.stream()))
    drain._submit()
    return a, m


def _sync_pack(hip, audio, mask, fmt, gain):
    """The synchronous path: the same pack into plain device tensors, copied back whole."""
    import torch
    a, m = torch.from_numpy(audio).cuda(), torch.from_numpy(mask).cuda()
    packed = torch.zeros((COUNT,) + SHAPE, dtype=torch.int16 if fmt == pcm_model.S16 else torch.float32, device="cuda")
    index = torch.zeros(COUNT, dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.check(hip.lib().rcfm_audio_pack(hip.ptr(a), hip.ptr(m), COUNT, ROW, fmt, gain, hip.ptr(packed), hip.ptr(index), hip.ptr(n),
                                        hip.stream()))
    k = int(n.cpu()[0])
    return index.cpu().numpy()[:k], packed.cpu().numpy()[:k]


@pytest.mark.parametrize("fmt,dtype", [(pcm_model.S16, "int16"), (pcm_model.F32, "float32")])
def test_three_buffers_through_depth_two(hip, fmt, dtype):
    """Three buffers with three different masks: handed out in order, bit-identical to the synchronous path and to the
    model, with the next buffer already submitted while one is read."""
    from radiocore.tools import Drain
    c = np.arange(COUNT)
    masks = [(c % 9 == 4).astype(np.uint8), np.where(c % 2 == 1, 255, 0).astype(np.uint8), (c % 7 != 0).astype(np.uint8)]
    audio = _buffers(masks)
    drain = Drain(COUNT, SHAPE, dtype, depth=2)
    assert (drain.depth, drain.rows, drain.row_shape, drain.dtype) == (2, COUNT, SHAPE, np.dtype(dtype))
    keep, got = [], []
    for i in range(3):
        keep.append(_submit(hip, drain, audio[i], masks[i], fmt, 32767.0))
        if i > 0:
            with drain.next() as (index, rows):
                got.append((index.copy(), rows.copy()))
    with drain.next() as (index, rows):
        got.append((index.copy(), rows.copy()))
    for i in range(3):
        want_index, want_rows, n = pcm_model.pack(audio[i], masks[i], fmt, 32767.0)
        assert 0 < n < COUNT
        sync_index, sync_rows = _sync_pack(hip, audio[i], masks[i], fmt, 32767.0)
        index, rows = got[i]
        assert index.dtype == np.int32 and rows.dtype == np.dtype(dtype) and rows.shape == (n,) + SHAPE, i
        assert np.array_equal(index, want_index) and np.array_equal(index, sync_index), i
        assert np.array_equal(pcm_model.bits(rows), pcm_model.bits(want_rows)), i
        assert np.array_equal(pcm_model.bits(rows), pcm_model.bits(sync_rows)), i
    drain.close()
    drain.close()                      # idempotent, like Feeder.close


def test_a_buffer_with_no_open_channel(hip):
    from radiocore.tools import Drain
    drain = Drain(COUNT, SHAPE, "int16", depth=2)
    mask = np.zeros(COUNT, np.uint8)
    keep = _submit(hip, drain, _buffers([mask])[0], mask, pcm_model.S16, 32767.0)
    with drain.next() as (index, rows):
        assert index.shape == (0,) and index.dtype == np.int32
        assert rows.shape == (0,) + SHAPE and rows.dtype == np.int16
    # the slot is free again and the next buffer comes out whole
    mask = np.ones(COUNT, np.uint8)
    audio = _buffers([mask], seed=3)[0]
    keep = _submit(hip, drain, audio, mask, pcm_model.S16, 32767.0)     # noqa: F841
    with drain.next() as (index, rows):
        assert np.array_equal(index, np.arange(COUNT, dtype=np.int32))
        assert np.array_equal(rows, pcm_model.q_s16(audio, 32767.0))
    drain.close()


def test_call_order_refusals(hip):
    """begin with every slot in flight and acquire / release with nothing submitted: RCFM_ERR_STATE, before any device call."""
    from radiocore.tools import Drain
    lib = hip.lib()
    drain = Drain(COUNT, SHAPE, "int16", depth=2)
    h = drain._handle.value
    n, v = ctypes.c_int(), ctypes.c_void_p()
    assert lib.rcfm_drain_acquire(h, ctypes.byref(n), ctypes.byref(v), ctypes.byref(v)) == ERR_STATE
    assert lib.rcfm_drain_release(h) == ERR_STATE
    with pytest.raises(RuntimeError):
        with drain.next():
            pass
    mask = np.ones(COUNT, np.uint8)
    audio = _buffers([mask])[0]
    keep = [_submit(hip, drain, audio, mask, pcm_model.S16, 32767.0) for _ in range(2)]     # noqa: F841
    assert lib.rcfm_drain_begin(h, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == ERR_STATE
    assert lib.rcfm_drain_submit(h, hip.stream()) == ERR_STATE
    with pytest.raises(RuntimeError, match="in flight"):
        drain._begin()
    assert lib.rcfm_drain_release(h) == ERR_STATE                       # submitted, but not acquired
    with drain.next() as (index, rows):
        assert rows.shape[0] == COUNT
    drain._begin()                                                      # one slot is free again
    with drain.next() as (index, rows):
        assert np.array_equal(rows, pcm_model.q_s16(audio, 32767.0))
    drain.close()


def test_close_with_a_copy_still_queued(hip):
    """close() right after a submit: destroy synchronises both copy streams before it frees the slots."""
    import torch
    from radiocore.tools import Drain
    drain = Drain(COUNT, SHAPE, "float32", depth=2)
    mask = np.ones(COUNT, np.uint8)
    keep = _submit(hip, drain, _buffers([mask])[0], mask, pcm_model.F32, 1.0)     # noqa: F841
    drain.close()
    assert drain._handle.value is None
    torch.cuda.synchronize()
    # and a drain that is dropped without close()
    drain = Drain(COUNT, SHAPE, "int16", depth=1)
    keep = _submit(hip, drain, _buffers([mask])[0], mask, pcm_model.S16, 32767.0)     # noqa: F841
    del drain
    torch.cuda.synchronize()


def test_drain_and_run_all_packed_refuse_a_mismatch(hip):
    import radiocore as rc
    from radiocore.tools import Drain
    with pytest.raises(ValueError):
        Drain(0, SHAPE)
    with pytest.raises(ValueError):
        Drain(COUNT, (0, 2))
    with pytest.raises(ValueError):
        Drain(COUNT, SHAPE, "int8")
    with pytest.raises(ValueError):
        Drain(COUNT, SHAPE, depth=0)
    N, B, A, C = 200_000, 25_000, 8_000, 8
    tuner = rc.Tuner()
    for i in range(C):
        tuner.add_channel(100e6 + B * i, B, rc.AM(B, A))
    tuner.request_bandwidth(float(N))
    tuner.load(np.zeros(N, np.complex64))
    for drain, pcm in ((Drain(C - 1, (A, 1)), rc.PCM()), (Drain(C, (A, 2)), rc.PCM()), (Drain(C, (A, 1)), rc.PCM("float32"))):
        with pytest.raises(ValueError):
            tuner.run_all_packed(pcm, drain=drain)
        drain.close()


def test_airband_pcm_example():
    """examples/airband_pcm.py at a reduced size: three buffers through run_all_packed(drain=) with depth 2; the example
    itself asserts every payload against the numpy quantisation of run_all's audio; only the planted channels publish."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("airband_pcm", os.path.join(ROOT, "examples", "airband_pcm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opened, planted, msgs = mod.run(channels=120, rate=4_000_000, buffers=3, stations=7)
    assert len(planted) == 3 and all(len(p) == 7 for p in planted)
    assert [sorted(o) for o in opened] == [sorted(p) for p in planted]
    assert len(msgs) == 21
    assert all(pcm.dtype == np.int16 and pcm.shape == (8000, 1) for _, pcm in msgs)
    assert max(int(np.abs(pcm).max()) for _, pcm in msgs) > 1000
