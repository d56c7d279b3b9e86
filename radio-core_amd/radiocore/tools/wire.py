"""Wire format of the reference's multi-channel server.

examples/multi_fm_server.py:103-106 publishes one ZeroMQ multipart message per channel and
buffer: [ int(center_frequency) as 4 little-endian bytes, float32 audio bytes ]; the client
(examples/multi_fm_receiver.py:23-24,47-49) subscribes on that 4-byte prefix.  FM / MFM
payloads are (A, 1) float32, WBFM payloads are (1, A, 2) float32 = interleaved L, R.
These helpers cut a batched [C, A, ch] audio block into those messages and back; the socket
itself (pyzmq) stays outside the package.
"""

import numpy as np

__all__ = ["frames", "frames_packed", "parse_frame"]


def frames(channels, audio, open_mask=None):
    """[(address_bytes, payload_bytes)] for a [C, A, ch] block, in channel order.  open_mask (bool [C], Tuner.open_mask):
    channels the squelch closed produce no message."""
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    if audio.ndim != 3 or audio.shape[0] != len(channels):
        raise ValueError("audio must be [channels, samples, audio_channels]")
    if open_mask is None:
        return [[ch.address_bytes, audio[i].tobytes()] for i, ch in enumerate(channels)]
    open_mask = np.asarray(open_mask, dtype=bool)
    if open_mask.shape != (len(channels),):
        raise ValueError("open_mask must hold one flag per channel")
    return [[ch.address_bytes, audio[i].tobytes()] for i, ch in enumerate(channels) if open_mask[i]]


def frames_packed(channels, index, audio):
    """[(address_bytes, payload_bytes)] for packed audio (Tuner.run_all_packed, Drain.next): row k of `audio`
    [n_open, A, ch] belongs to channel index[k], and the payload is the row's bytes in its own dtype (int16 PCM, or float32).
    Channels that are not listed produce no message."""
    audio = np.asarray(audio)
    index = np.asarray(index)
    if audio.ndim != 3 or index.ndim != 1 or index.shape[0] != audio.shape[0]:
        raise ValueError("audio must be [listed channels, samples, audio_channels] with one index per row")
    return [[channels[int(c)].address_bytes, np.ascontiguousarray(audio[k]).tobytes()] for k, c in enumerate(index)]


def parse_frame(message, audio_channels, dtype=np.float32):
    """(center frequency in Hz, `dtype` [A, audio_channels]) from one multipart message (dtype: float32 as the reference
    sends it, int16 for frames_packed of PCM audio)."""
    address, payload = message
    freq = int.from_bytes(address, byteorder="little")
    pcm = np.frombuffer(payload, dtype=dtype)
    return freq, pcm.reshape(-1, audio_channels)
