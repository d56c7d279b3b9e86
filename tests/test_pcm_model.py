"""CPU: the numpy model of the audio egress (tests/pcm_model.py) against the definition in include/rcfm.h, case by case,
and the frames_packed / parse_frame(dtype=) round trip.  The GPU tests (test_hip_pcm.py) hold the kernel to this model."""

import numpy as np
import pytest

import pcm_model

MASKS = {
    "all_open": lambda n: np.ones(n, np.uint8),
    "all_closed": lambda n: np.zeros(n, np.uint8),
    "alternating": lambda n: (np.arange(n) % 2).astype(np.uint8),
    "first_only": lambda n: (np.arange(n) == 0).astype(np.uint8),
    "last_only": lambda n: (np.arange(n) == n - 1).astype(np.uint8),
    "bytes_255": lambda n: np.where(np.arange(n) % 3 == 1, 255, 0).astype(np.uint8),
}


def test_rounding_is_to_nearest_even_on_exact_ties():
    """gain = 32768 is a power of two: (k + 0.5) / 32768 is exact in float32 and so is the product back."""
    gain = 32768.0
    k = np.array([0, 1, 2, 3, 4, 5, 100, 101, 32765, 32766, -1, -2, -3, -4, -101, -32766, -32767], np.float64)
    x = ((k + 0.5) / gain).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * gain, k + 0.5)               # the ties are exact
    want = np.where(np.floor(k) % 2 == 0, k, k + 1).astype(np.int16)           # k + 0.5 -> the even neighbour
    assert np.array_equal(pcm_model.q_s16(x, gain), want)
    # with 32767 the same inputs are no ties: the model still rounds the float32 product, whatever it is
    y = x * np.float32(32767.0)
    assert np.array_equal(pcm_model.q_s16(x, 32767.0), np.rint(y).astype(np.int16))


def test_saturation_is_symmetric():
    x = np.array([1.0, -1.0, 1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20, 1.5, -1.5, 3e38, -3e38, 32767.4 / 32767, 0.99998], np.float32)
    got = pcm_model.q_s16(x, 32767.0)
    assert got[:8].tolist() == [32767, -32767, 32767, -32767, 32767, -32767, 32767, -32767]
    assert got.min() == -32767 and got.max() == 32767
    # a product that overflows float32 saturates, and -32768 never appears even where y = -32768 exactly
    assert pcm_model.q_s16(np.array([3e38, -3e38, -1.0], np.float32), 32768.0).tolist() == [32767, -32767, -32767]
    assert pcm_model.q_s16(np.array([-32768.0, -40000.0], np.float32), 1.0).tolist() == [-32767, -32767]


def test_nan_inf_and_denormals():
    nan2 = np.array([0x7fc00001, 0xffc12345], np.uint32).view(np.float32)
    x = np.concatenate([nan2, np.array([np.inf, -np.inf, 0.0, -0.0], np.float32)])
    assert pcm_model.q_s16(x, 32767.0).tolist() == [0, 0, 32767, -32767, 0, 0]
    # denormal inputs: times the largest allowed gain they stay below 2^-102 and round to 0, flushed or not
    den = np.array([1, 0x7fffff, 0x80000001, 0x807fffff], np.uint32).view(np.float32)
    assert np.all(den != 0) and np.all(np.abs(den) < np.finfo(np.float32).tiny)
    for gain in (1.0, 32767.0, 2.0 ** 24):
        assert pcm_model.q_s16(den, gain).tolist() == [0, 0, 0, 0]
    # float32 passes the bits, NaN payloads included
    _, packed, _ = pcm_model.pack(x[None], None, pcm_model.F32, 1.0)
    assert np.array_equal(pcm_model.bits(packed[0]), pcm_model.bits(x))


@pytest.mark.parametrize("name", sorted(MASKS))
@pytest.mark.parametrize("n", [1, 2, 7, 256])
def test_slots_index_and_n_open(name, n):
    mask = MASKS[name](n)
    slot, index, n_open = pcm_model.slots(mask)
    is_open = mask != 0
    assert n_open == int(is_open.sum()) == index.shape[0]
    assert slot.dtype == np.int32 and index.dtype == np.int32
    for c in range(n):
        if is_open[c]:
            assert slot[c] == int(is_open[:c].sum())          # the number of open channels below c
            assert index[slot[c]] == c
        else:
            assert slot[c] == -1
    assert np.all(np.diff(index) > 0)                         # channel order is kept
    if name == "all_open":
        assert index.tolist() == list(range(n))
        assert np.array_equal(pcm_model.slots(None, n)[1], index)
    if name == "all_closed":
        assert n_open == 0
    if name == "first_only":
        assert index.tolist() == [0]
    if name == "last_only":
        assert index.tolist() == [n - 1]


def test_pack_rows_follow_the_index():
    rng = np.random.default_rng(5)
    audio = (0.5 * rng.standard_normal((6, 9, 2))).astype(np.float32)
    mask = np.array([0, 255, 1, 0, 0, 7], np.uint8)
    index, packed, n = pcm_model.pack(audio, mask, pcm_model.S16, 32767.0)
    assert n == 3 and index.tolist() == [1, 2, 5] and packed.shape == (3, 9, 2) and packed.dtype == np.int16
    for k, c in enumerate(index):
        assert np.array_equal(packed[k], pcm_model.q_s16(audio[c], 32767.0))
    index, packed, n = pcm_model.pack(audio, mask, pcm_model.F32, 32767.0)
    assert packed.dtype == np.float32 and np.array_equal(pcm_model.bits(packed), pcm_model.bits(audio[[1, 2, 5]]))


def test_frames_packed_round_trip():
    from radiocore.tools import wire
    from radiocore.tools.tuner import Channel
    channels = [Channel(i, 25000.0, None, 0.0, 118_012_500.0 + 25000.0 * i, 0.0) for i in range(6)]
    rng = np.random.default_rng(9)
    audio = (0.5 * rng.standard_normal((6, 40, 2))).astype(np.float32)
    mask = np.array([1, 0, 0, 1, 1, 0], np.uint8)
    for fmt, dtype in ((pcm_model.S16, np.int16), (pcm_model.F32, np.float32)):
        index, packed, n = pcm_model.pack(audio, mask, fmt, 32767.0)
        msgs = wire.frames_packed(channels, index, packed)
        assert msgs == pcm_model.frame_payloads([c.address_bytes for c in channels], index, packed)
        assert len(msgs) == n == 3                                   # closed channels produce no message
        for k, m in enumerate(msgs):
            assert len(m[1]) == 40 * 2 * np.dtype(dtype).itemsize
            freq, pcm = wire.parse_frame(m, 2, dtype=dtype)
            assert freq == int(channels[index[k]].center_frequency)
            assert pcm.dtype == dtype and pcm.shape == (40, 2) and np.array_equal(pcm, packed[k])
    # the default of parse_frame is what it was: float32
    msg = wire.frames(channels[:1], audio[:1])[0]
    freq, pcm = wire.parse_frame(msg, 2)
    assert pcm.dtype == np.float32 and np.array_equal(pcm, audio[0])
    assert wire.frames_packed(channels, np.zeros(0, np.int32), np.zeros((0, 40, 2), np.int16)) == []
    with pytest.raises(ValueError):
        wire.frames_packed(channels, index, packed[:2])
