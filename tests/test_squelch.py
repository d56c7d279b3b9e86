"""CPU: the signal-level definition (tests/squelch_model.py against radiocore_oracle.Tuner), the two entry points'
declarations and NULL checks, and the host-side pieces of the squelch (thresholds, wire frames, the Tuner's methods).
The kernels are tested under -m gpu (tests/test_hip_squelch.py)."""

import ctypes
import os
import re

import numpy as np
import pytest

import radiocore_oracle as oracle
import squelch_model
from conftest import ROOT

LIB = os.path.join(ROOT, "radio-core_amd", "radiocore", "_lib", "librcfm.so")


# ---- 1. the model is the Parseval sum of the oracle's channel ------------------------------------------------------

GEOMETRIES = {
    # name: (N, [(centre offset from 50 MHz, bandwidth)])
    "even_B": (60000, [(0, 20000), (21000, 20000)]),
    "odd_B": (90001, [(0, 30000), (20000, 20001)]),                    # the tuner_odd fixture's geometry
    "mixed": (120000, [(0, 48000), (30250, 12500), (42750, 12500), (52000, 6001)]),
    "small_N": (64, [(0, 16), (17, 15), (30, 2), (33, 1), (40, 8)]),
    "B_equals_N": (48, [(0, 48)]),
}


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_model_level_is_mean_power_of_the_channel(name):
    N, chans = GEOMETRIES[name]
    t = oracle.Tuner()
    for off, bw in chans:
        t.add_channel(50e6 + off, bw, None)
    t.request_bandwidth(float(N))
    rng = np.random.default_rng(len(name))
    x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
    x += 3.0 * np.exp(2j * np.pi * 7 * np.arange(N) / N)
    t.load(x.astype(np.complex128))           # float64 throughout (numpy transforms complex64 in single precision)
    lv = squelch_model.levels(oracle, t)
    for i in range(len(chans)):
        want = float(np.mean(np.abs(t.run_pruned(i)) ** 2))
        assert want > 0
        assert abs(lv[i] - want) <= 1e-12 * want, (name, i, lv[i], want)


def test_model_mask_rule():
    lv = np.array([1.0, 2.0, np.nan, 3.0, 0.0])
    th = np.array([1.0, 2.5, 1.0, np.nan, 0.0])
    assert squelch_model.open_mask(lv, th).tolist() == [True, False, False, False, True]


# ---- 2., 3. the ABI ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_entry_points_are_declared_exported_and_bound(lib):
    from radiocore._internal import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rcfm.h")).read(), flags=re.S)
    for name in ("rcfm_tuner_levels", "rcfm_squelch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES, name
    assert len(hip.SIGNATURES["rcfm_tuner_levels"]) == 5 and len(hip.SIGNATURES["rcfm_squelch"]) == 7


def test_null_arguments_need_no_device(lib):
    assert lib.rcfm_tuner_levels(None, 0, 0, None, None) == -4
    assert lib.rcfm_squelch(None, None, 1, ctypes.c_size_t(1), None, None, None) == -4


def test_profile_stages_are_appended(lib):
    lib.rcfm_profile_stage_name.restype = ctypes.c_char_p
    names = [lib.rcfm_profile_stage_name(i).decode() for i in range(lib.rcfm_profile_stage_count())]
    assert names[-2:] == ["levels", "squelch"] and names.index("ssb_tail") == len(names) - 3
    assert names[0] == "tuner_fft_N"          # the existing indices did not move


# ---- 4. host-side pieces -------------------------------------------------------------------------------------------

def test_threshold_over_floor_arithmetic():
    from radiocore.tools import squelch
    bw = np.array([25000.0] * 6 + [12500.0] * 3)
    lv = np.array([2.5e-11, 2.6e-11, 2.4e-11, 0.3, 2.5e-11, 0.02, 1.25e-11, 1.2e-11, 0.5])
    thr = squelch.threshold_over_floor(lv, bw, 10.0)
    density = np.median(lv / bw)
    assert density == pytest.approx(1e-15, rel=0.05)
    assert thr.dtype == np.float32 and thr.shape == (9,)
    np.testing.assert_allclose(thr, density * bw * 10.0, rtol=1e-6)
    assert (lv >= thr).tolist() == [False, False, False, True, False, True, False, False, True]
    # a scalar bandwidth, and 0 dB = the floor itself
    np.testing.assert_allclose(squelch.threshold_over_floor(lv[:6], 25000, 0.0), np.full(6, np.median(lv[:6])), rtol=1e-6)
    with pytest.raises(ValueError):
        squelch.threshold_over_floor([], [], 10.0)
    with pytest.raises(ValueError):
        squelch.threshold_over_floor([1.0], [0.0], 10.0)
    import radiocore.tools
    assert radiocore.tools.threshold_over_floor is squelch.threshold_over_floor


def test_wire_frames_with_and_without_a_mask():
    from radiocore.tools import wire
    chans = [oracle.Channel(i, 25000, None, 118e6 + 25000 * i) for i in range(5)]
    audio = np.arange(5 * 8, dtype=np.float32).reshape(5, 8, 1)
    every = wire.frames(chans, audio)
    assert len(every) == 5 and every == wire.frames(chans, audio, open_mask=None)
    mask = np.array([True, False, False, True, False])
    some = wire.frames(chans, audio, open_mask=mask)
    assert len(some) == 2
    for message, i in zip(some, (0, 3)):
        freq, pcm = wire.parse_frame(message, 1)
        assert freq == int(chans[i].center_frequency)
        assert np.array_equal(pcm, audio[i])
    assert wire.frames(chans, audio, open_mask=np.zeros(5, bool)) == []
    with pytest.raises(ValueError):
        wire.frames(chans, audio, open_mask=[True, False])


def test_tuner_and_lanes_carry_the_squelch_interface():
    """(A Tuner cannot be constructed without a device: the methods are checked on the class.)"""
    import inspect
    from radiocore.tools import Lanes, Tuner
    for name in ("levels", "set_squelch", "open_mask"):
        assert callable(getattr(Tuner, name)), name
    assert inspect.signature(Tuner.set_squelch).parameters["threshold"].default is None
    assert inspect.signature(Tuner.levels).parameters["numpy_output"].default is True
    sig = inspect.signature(Lanes.result).parameters
    assert sig["open_mask"].default is False and sig["numpy_output"].default is True
