"""CPU: the raw-IQ conversions (tests/iq_model.py) are exact for every value of each type, the headers declare the formats
and the three entry points, the binding table has them, and the argument errors that need no device."""

import ctypes
import os
import re

import numpy as np
import pytest

import iq_model
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rcfm.h")
TOOLS_HEADER = os.path.join(ROOT, "include", "rcfm_tools.h")
LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")
ERR_ARG = -4


@pytest.mark.parametrize("dtype", ["int16", "int8", "uint8"])
def test_every_value_converts_exactly(dtype):
    v = iq_model.all_values(np.dtype(dtype))
    assert v.size == (65536 if dtype == "int16" else 256)
    f = iq_model.to_float32(v)
    assert f.dtype == np.float32
    assert np.array_equal(f.astype(np.float64), iq_model.exact_float64(v))
    assert float(np.max(np.abs(f))) <= 1.0


def test_the_documented_end_points():
    assert iq_model.to_float32(np.array([-32768, 32767], np.int16)).tolist() == [-1.0, 32767 / 32768]
    assert iq_model.to_float32(np.array([-128, 127], np.int8)).tolist() == [-1.0, 127 / 128]
    assert iq_model.to_float32(np.array([0, 255], np.uint8)).tolist() == [-0.99609375, 0.99609375]


def test_pairs_interleave_i_then_q():
    raw = np.array([[16384, -16384], [0, 32767]], np.int16)
    want = np.array([0.5 - 0.5j, 0 + (32767 / 32768) * 1j], np.complex64)
    assert np.array_equal(iq_model.to_complex64(raw), want)
    assert np.array_equal(iq_model.to_complex64(raw.reshape(-1)), want)
    with pytest.raises(ValueError):
        iq_model.to_float32(np.zeros(4, np.int32))


def test_random_pairs_plant_the_extremes():
    for fmt, dt in iq_model.DTYPES.items():
        info = np.iinfo(dt)
        x = iq_model.random_pairs(fmt, 100, 1, line=16)
        assert x.dtype == dt and x.shape == (100, 2)
        assert x[0].tolist() == [info.min, info.max] and x[1].tolist() == [info.max, info.min]
        assert x[99].tolist() == [info.min, info.max] and x[16].tolist() == [info.max, info.min]


def _uncommented(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_headers_declare_formats_and_entry_points():
    host, tools = _uncommented(HEADER), _uncommented(TOOLS_HEADER)
    assert re.search(r"enum\s*\{\s*RCFM_IQ_CS16\s*=\s*1\s*,\s*RCFM_IQ_CS8\s*=\s*2\s*,\s*RCFM_IQ_CU8\s*=\s*3\s*\}", host)
    assert re.search(r"int\s+rcfm_tuner_load_raw\s*\(\s*rcfm_tuner_t\s+t\s*,\s*int\s+format\s*,\s*const\s+void\s*\*\s*x\s*,"
                     r"\s*void\s*\*\s*stream\s*\)\s*;", host)
    assert re.search(r"int\s+rcfm_iq_convert\s*\(\s*int\s+format\s*,\s*size_t\s+n\s*,\s*const\s+void\s*\*\s*in\s*,"
                     r"\s*void\s*\*\s*out_c64\s*,\s*void\s*\*\s*stream\s*\)\s*;", host)
    assert re.search(r"int\s+rcfm_tuner_load_route\s*\(\s*rcfm_tuner_t\s+t\s*,\s*int\s+format\s*,\s*int\s*\*\s*route\s*\)\s*;",
                     tools)
    assert "rcfm_tuner_load_route" not in host
    assert re.search(r"#define\s+RCFM_VERSION\s+102\b", host)


def test_binding_table_has_the_new_symbols():
    from radiocore._internal import hip
    assert len(hip.SIGNATURES["rcfm_tuner_load_raw"]) == 4
    assert len(hip.SIGNATURES["rcfm_iq_convert"]) == 5
    assert len(hip.SIGNATURES["rcfm_tuner_load_route"]) == 3
    assert (hip.RCFM_IQ_CS16, hip.RCFM_IQ_CS8, hip.RCFM_IQ_CU8) == (1, 2, 3)
    assert (iq_model.RCFM_IQ_CS16, iq_model.RCFM_IQ_CS8, iq_model.RCFM_IQ_CU8) == (1, 2, 3)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_argument_errors_need_no_device(lib):
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.rcfm_tuner_load_raw.argtypes = [vp, ctypes.c_int, vp, vp]
    lib.rcfm_tuner_load_route.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.rcfm_iq_convert.argtypes = [ctypes.c_int, sz, vp, vp, vp]
    lib.rcfm_last_error.restype = ctypes.c_char_p
    route = ctypes.c_int(-7)
    some = ctypes.create_string_buffer(64)             # never dereferenced: every call below fails before it
    p = ctypes.cast(some, vp)
    for fmt in (1, 2, 3):
        assert lib.rcfm_tuner_load_raw(None, fmt, p, None) == ERR_ARG            # NULL handle
        assert lib.rcfm_tuner_load_route(None, fmt, ctypes.byref(route)) == ERR_ARG
        assert lib.rcfm_iq_convert(fmt, sz(0), None, None, None) == 0            # n = 0: a no-op, NULL pointers and all
        assert lib.rcfm_iq_convert(fmt, sz(4), None, None, None) == ERR_ARG
    for fmt in (0, 4, -1):
        assert lib.rcfm_tuner_load_raw(None, fmt, p, None) == ERR_ARG
        assert b"format" in lib.rcfm_last_error()
        assert lib.rcfm_tuner_load_raw(p, fmt, p, None) == ERR_ARG               # the format is looked at first: `p` is no handle
        assert lib.rcfm_tuner_load_route(p, fmt, ctypes.byref(route)) == ERR_ARG
        assert lib.rcfm_iq_convert(fmt, sz(0), None, None, None) == ERR_ARG
        assert lib.rcfm_iq_convert(fmt, sz(4), p, p, None) == ERR_ARG
        assert b"format" in lib.rcfm_last_error()
    assert route.value == -7
