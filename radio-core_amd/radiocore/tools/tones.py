"""Signalling tones on the audio, host side (no reference counterpart): the CTCSS and SELCAL tables, and what turns the
tone bank's powers (``Tuner.tone_power``: P [C, F, K], E [C, F]) into a detected tone or a SELCAL code.  numpy only."""

import numpy as np

__all__ = ["CTCSS", "SELCAL", "SELCAL_LETTERS", "strongest", "selcal_code"]

# The 39 standard CTCSS tones, Hz
CTCSS = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8,
         123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 162.2, 167.9, 173.8, 179.9, 186.2, 192.8, 203.5, 210.7,
         218.1, 225.7, 233.6, 241.8, 250.3)

# The 16 SELCAL tones, Hz, in the order of their letters (I, N and O are not used)
SELCAL_LETTERS = "ABCDEFGHJKLMPQRS"
SELCAL = (312.6, 346.7, 384.6, 426.6, 473.2, 524.8, 582.1, 645.7, 716.1, 794.3, 881.0, 977.2, 1083.9, 1202.3, 1333.5, 1479.1)


def strongest(P, E, ratio, n=1):
    """int [C, F, n]: per channel and frame the indices of the up to ``n`` strongest tones whose share of the frame's
    power ``P / E`` is at least ``ratio``, strongest first, -1 where there is none (frames with ``E == 0`` have none; of
    equal shares the lower index comes first).  P: [C, F, K], E: [C, F]."""
    P = np.asarray(P, dtype=np.float64)
    E = np.asarray(E, dtype=np.float64)
    if P.ndim != 3 or E.shape != P.shape[:2]:
        raise ValueError("strongest: P is [C, F, K] and E is [C, F]")
    n = int(n)
    if n < 1 or n > P.shape[2]:
        raise ValueError("strongest: n is 1 .. K")
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(E[..., None] > 0, P / E[..., None], 0.0)
    share = np.where(np.isnan(share), 0.0, share)
    order = np.argsort(-share, axis=2, kind="stable")[..., :n]
    top = np.take_along_axis(share, order, axis=2)
    return np.where(top >= ratio, order, -1).astype(np.int64)


def selcal_code(frames, min_frames=1):
    """A SELCAL call from a time series of the strongest two tones per frame: ``frames`` is a sequence of index pairs into
    ``SELCAL`` (``strongest(P, E, ratio, n=2)[c]``, possibly of several buffers one after the other); a frame with a -1
    is silence.  A call is two different tone pairs, each held for at least ``min_frames`` consecutive frames; the code is
    ``"AB-CD"``, the letters of a pair in alphabetical order.  None when the series holds no complete call."""
    runs = []                               # [pair, frames it lasted]
    prev = None
    for fr in frames:
        a, b = int(fr[0]), int(fr[1])
        pair = (min(a, b), max(a, b)) if a >= 0 and b >= 0 and a != b else None
        if pair is not None and pair == prev:
            runs[-1][1] += 1
        elif pair is not None:
            runs.append([pair, 1])
        prev = pair
    held = []
    for pair, count in runs:
        if count >= min_frames and (not held or held[-1] != pair):
            held.append(pair)
    if len(held) < 2:
        return None
    return "-".join(SELCAL_LETTERS[p[0]] + SELCAL_LETTERS[p[1]] for p in held[:2])
