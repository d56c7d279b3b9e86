"""CPU: the audio egress entry points (include/rcfm.h: rcfm_audio_pack, rcfm_drain_*) -- declared, exported, bound, and
refusing bad arguments before any device call -- and the validation of radiocore.PCM."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
NEW = ("rcfm_audio_pack", "rcfm_drain_create", "rcfm_drain_begin", "rcfm_drain_submit", "rcfm_drain_acquire",
       "rcfm_drain_release", "rcfm_drain_destroy")
_f = ctypes.c_float
_sz = ctypes.c_size_t
ERR_ARG = -4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.rcfm_last_error.restype = ctypes.c_char_p
    return lib


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert len(hip.SIGNATURES["rcfm_audio_pack"]) == 10 and len(hip.SIGNATURES["rcfm_drain_acquire"]) == 4
    assert re.search(r"RCFM_PCM_F32\s*=\s*0\b", header) and re.search(r"RCFM_PCM_S16\s*=\s*1\b", header)
    assert (hip.RCFM_PCM_F32, hip.RCFM_PCM_S16) == (0, 1)
    # the segment length the GPU tests straddle is the kernel's own
    kernel = open(os.path.join(ROOT, "radio-core_amd", "csrc", "egress_kernel.h")).read()
    assert re.search(r"kPackThreads\s*=\s*256\b", kernel) and re.search(r"kPackSegment\s*=\s*16\s*\*\s*kPackThreads\b", kernel)
    assert hip.RCFM_PACK_SEGMENT == 16 * 256
    assert lib.rcfm_version() == 102


def test_audio_pack_refuses_bad_arguments_without_a_device(lib):
    a = ctypes.c_void_p(0x100000)          # never dereferenced: every call below is refused on the host
    p = ctypes.c_void_p(0x800000)
    S16, F32 = 1, 0

    def call(audio=a, open_=None, count=3, row=100, fmt=S16, gain=32767.0, packed=p, index=None, n_open=None):
        return lib.rcfm_audio_pack(audio, open_, count, _sz(row), fmt, _f(gain), packed, index, n_open, None)
    bad = [dict(audio=None), dict(packed=None), dict(count=0), dict(count=-1), dict(count=65536), dict(row=0),
           dict(fmt=2), dict(fmt=-1),
           dict(gain=0.0), dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=2.0 ** 24 + 2.0),
           dict(packed=a),                                              # the same buffer
           dict(packed=ctypes.c_void_p(0x100000 + 2 * 100)),             # packed starts inside audio
           dict(packed=ctypes.c_void_p(0x100000 + 4 * 300 - 2)),         # ... in its last sample
           dict(packed=ctypes.c_void_p(0x100000 - 2)),                   # audio starts inside packed (its last row)
           dict(fmt=F32, packed=ctypes.c_void_p(0x100000 - 4 * 300 + 4)),
           dict(fmt=F32, packed=ctypes.c_void_p(0x100000 + 4 * 299)),
           dict(audio=ctypes.c_void_p(0x100002)), dict(packed=ctypes.c_void_p(0x800001)),      # not aligned for an element
           dict(fmt=F32, packed=ctypes.c_void_p(0x800002))]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert call(count=65536) == ERR_ARG and b"65535" in lib.rcfm_last_error()
    assert call(packed=a) == ERR_ARG and b"overlap" in lib.rcfm_last_error()
    assert call(gain=0.0) == ERR_ARG and b"gain" in lib.rcfm_last_error()
    assert call(fmt=7) == ERR_ARG and b"format" in lib.rcfm_last_error()


def test_drain_refuses_bad_arguments_without_a_device(lib):
    out = ctypes.c_void_p()

    def create(row_bytes=1024, max_rows=8, depth=2, out_=ctypes.byref(out)):
        return lib.rcfm_drain_create(_sz(row_bytes), max_rows, depth, out_)
    for kw in (dict(row_bytes=0), dict(max_rows=0), dict(max_rows=-1), dict(max_rows=65536), dict(depth=0), dict(depth=-1),
               dict(out_=None)):
        assert create(**kw) == ERR_ARG, kw
    assert out.value is None
    v = ctypes.c_void_p()
    n = ctypes.c_int()
    assert lib.rcfm_drain_begin(None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == ERR_ARG
    assert lib.rcfm_drain_submit(None, None) == ERR_ARG
    assert lib.rcfm_drain_acquire(None, ctypes.byref(n), ctypes.byref(v), ctypes.byref(v)) == ERR_ARG
    assert lib.rcfm_drain_release(None) == ERR_ARG
    assert lib.rcfm_drain_destroy(None) == 0           # like free(NULL) and rcfm_feeder_destroy(NULL)


def test_run_all_packed_call_order_with_a_drain(monkeypatch):
    """The Python layer with the ABI replaced by a counting stand-in: run_all's launch, then begin / pack / submit on the
    drain's slot, nothing returned; a drain of the wrong geometry is refused before anything is launched."""
    from test_am import _CountingLib, _FakeTensor, _FakeTorch
    from radiocore._internal import hip
    lib = _CountingLib()
    monkeypatch.setattr(hip, "lib", lambda: lib)
    monkeypatch.setattr(hip, "torch", lambda: _FakeTorch)
    monkeypatch.setattr(hip, "empty", lambda shape, dtype: _FakeTensor(shape))
    monkeypatch.setattr(hip, "ptr", lambda t: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(hip, "to_device", lambda x, dtype=None: _FakeTensor(getattr(x, "shape", (len(x),))))
    import radiocore as rc
    from radiocore.tools import Drain
    B, A, C = 25000, 8000, 6
    tuner = rc.Tuner()
    for i in range(C):
        tuner.add_channel(118.0e6 + float(B) * i, B, rc.AM(B, A))
    tuner.request_bandwidth(600_000.0)
    tuner.load(np.zeros(600_000, np.complex64))
    drain = Drain(C, (A, 1), "int16", depth=2)
    assert lib.count("rcfm_drain_create") == 1
    create = [a for n, a in lib.calls if n == "rcfm_drain_create"][0]
    assert tuple(create[:3]) == (A * 2, C, 2)
    lib.calls.clear()
    assert tuner.run_all_packed(rc.PCM("int16", 8192.0), drain=drain) is None
    names = [n for n, _ in lib.calls if n.startswith(("rcfm_pipeline", "rcfm_audio", "rcfm_drain"))]
    assert names == ["rcfm_drain_begin", "rcfm_pipeline_run", "rcfm_audio_pack", "rcfm_drain_submit"]
    pack = [a for n, a in lib.calls if n == "rcfm_audio_pack"][0]
    assert pack[1] is None and tuple(pack[2:6]) == (C, A, hip.RCFM_PCM_S16, 8192.0)          # squelch off: open = NULL
    lib.calls.clear()
    for bad, pcm in ((Drain(C - 1, (A, 1)), rc.PCM()), (Drain(C, (A, 2)), rc.PCM()), (drain, rc.PCM("float32"))):
        with pytest.raises(ValueError):
            tuner.run_all_packed(pcm, drain=bad)
    assert lib.count("rcfm_pipeline_run") == 0 and lib.count("rcfm_audio_pack") == 0


def test_pcm_validates_like_the_abi():
    import radiocore as rc
    from radiocore._internal import hip
    from radiocore.tools import PCM
    assert rc.PCM is PCM
    p = rc.PCM()
    assert p.dtype == np.dtype("int16") and p.gain == 32767.0 and p.format == hip.RCFM_PCM_S16
    assert rc.PCM("int16", 32768).gain == 32768.0 and rc.PCM(np.int16, 2.0 ** 24).gain == 2.0 ** 24
    f = rc.PCM(dtype="float32")
    assert f.dtype == np.dtype("float32") and f.format == hip.RCFM_PCM_F32
    rc.PCM("float32", gain=0.0)                        # gain is ignored for float32, as in the ABI
    for bad in (dict(gain=0.0), dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=2.0 ** 24 + 2.0),
                dict(gain=1e39), dict(gain="loud"), dict(dtype="int8"), dict(dtype="float64"), dict(dtype="pcm")):
        with pytest.raises(ValueError):
            rc.PCM(**bad)
    assert "int16" in repr(p)
