"""numpy model of the audio egress (include/rcfm.h, "audio egress"): the slots, index and n_open of a mask, the
conversion q, the packed rows, and the frames a publisher makes of them.  The GPU tests compare bit for bit against it."""

import numpy as np

F32, S16 = 0, 1          # RCFM_PCM_F32, RCFM_PCM_S16


def slots(open_mask, count=None):
    """(slot int32 [count] with -1 for closed channels, index int32 [n_open], n_open).  open_mask: [count] bytes, any
    nonzero byte is open; None: every channel of `count` is open."""
    is_open = np.ones(int(count), bool) if open_mask is None else np.asarray(open_mask) != 0
    index = np.flatnonzero(is_open).astype(np.int32)
    slot = np.full(is_open.shape[0], -1, np.int32)
    slot[index] = np.arange(index.shape[0], dtype=np.int32)
    return slot, index, int(index.shape[0])


def q_s16(x, gain):
    """RCFM_PCM_S16: y = x * gain in float32; NaN -> 0; else round to nearest even, clamp to [-32767, 32767]."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = x * np.float32(gain)
        assert y.dtype == np.float32
        r = np.clip(np.rint(y), np.float32(-32767.0), np.float32(32767.0))
        return np.where(np.isnan(y), np.float32(0.0), r).astype(np.int16)


def q(x, fmt, gain):
    """q of the format: int16 for S16; for F32 the float32 array itself (compare its bits as uint32)."""
    if fmt == S16:
        return q_s16(x, gain)
    if fmt != F32:
        raise ValueError("unknown format")
    return np.asarray(x, np.float32)


def pack(audio, open_mask, fmt, gain):
    """(index int32 [n_open], packed [n_open, ...], n_open) of audio [count, ...] float32."""
    audio = np.asarray(audio, np.float32)
    _, index, n = slots(open_mask, audio.shape[0])
    rows = audio[index]
    if fmt == F32:
        return index, rows.copy(), n
    return index, q_s16(rows, gain), n


def bits(a):
    """An array as unsigned integers of its element size: equality of these is bit identity (NaN payloads included)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def frame_payloads(addresses, index, packed):
    """[(address_bytes, payload_bytes)]: one message per listed channel, the payload the row's bytes in its dtype."""
    return [[addresses[int(c)], np.ascontiguousarray(packed[k]).tobytes()] for k, c in enumerate(index)]
