"""Raw integer IQ as receivers deliver it (include/rcfm.h, RCFM_IQ_*; no reference counterpart: the reference takes
complex64 only): interleaved I, Q, full scale 1.0 -- int16 (Airspy, the USRP wire format, most files), int8 (HackRF),
uint8 (RTL-SDR, centre 127.5).  ``Tuner.load_raw`` takes such a buffer as it is; ``to_complex64`` is the conversion alone,
for ``Decimate`` / ``WBFM.run`` or code of the caller's own.  Both give the same float32 values, each exactly the integer
times its power of two.

The receivers that deliver int8 and uint8 are the ones with IQ imbalance: ``impair`` is the receiver model, and
``balance_from`` the calibrate-occasionally recipe for ``Tuner.set_iq_balance`` -- the counterpart of
``squelch.threshold_over_floor`` for ``Tuner.set_squelch``: ``Tuner.iq_imbalance()`` on a few buffers (over a frequency
range without mirrored carriers), ``balance_from`` of what it returned, and the one beta set as a fixed balance.
"""

import ctypes

import numpy as np

from radiocore._internal import hip

__all__ = ["to_complex64", "FORMATS", "impair", "imbalance", "beta_from_sums", "balance_from", "pair_range"]

FORMATS = {np.dtype("int16"): hip.RCFM_IQ_CS16, np.dtype("int8"): hip.RCFM_IQ_CS8, np.dtype("uint8"): hip.RCFM_IQ_CU8}


# ---- IQ imbalance (include/rcfm.h, "IQ balance"; Tuner.iq_imbalance / Tuner.set_iq_balance).  Host numpy only. ----------

def imbalance(gain, phase):
    """(mu, nu, beta) of a receiver whose Q path has `gain` times the amplitude of its I path and `phase` radians of
    quadrature error: x' = mu x + nu conj(x), mu = (1 + g e^{-j phi}) / 2, nu = (1 - g e^{j phi}) / 2, and
    beta = nu / conj(mu) is what ``Tuner.set_iq_balance`` removes the image with."""
    g, phi = float(gain), float(phase)
    mu = (1.0 + g * np.exp(-1j * phi)) / 2.0
    nu = (1.0 - g * np.exp(1j * phi)) / 2.0
    return complex(mu), complex(nu), complex(nu / np.conj(mu))


def impair(x, gain, phase):
    """complex128 mu x + nu conj(x): what the receiver of ``imbalance(gain, phase)`` delivers for the true baseband x."""
    mu, nu, _ = imbalance(gain, phase)
    x = np.asarray(x, dtype=np.complex128)
    return mu * x + nu * np.conj(x)


def beta_from_sums(sums):
    """beta of (Re P, Im P, Q), the finish step of rcfm_tuner_iq_estimate in float64: c = 2 P / Q,
    beta = c / (1 + sqrt(1 - min(|c|^2, 1))); 0 when Q is not positive or anything is not finite."""
    pr, pi, q = (float(v) for v in np.asarray(sums, dtype=np.float64).reshape(3))
    if not (q > 0.0 and np.isfinite(pr) and np.isfinite(pi) and np.isfinite(q)):
        return 0j
    cr, ci = (2.0 * pr) / q, (2.0 * pi) / q
    d = 1.0 + np.sqrt(1.0 - min(cr * cr + ci * ci, 1.0))
    beta = complex(cr / d, ci / d)
    return beta if np.isfinite(beta.real) and np.isfinite(beta.imag) else 0j


def balance_from(estimates):
    """One beta from several buffers: calibrate occasionally, correct every buffer.  `estimates` holds what
    ``Tuner.iq_imbalance`` returned for each of them -- ``(beta, sums)`` pairs, or the ``sums`` = (Re P, Im P, Q) alone; the
    sums add up (a strong buffer weighs more, as it should) and the result is the beta of the totals, to hand to
    ``Tuner.set_iq_balance``.  ValueError for an empty list."""
    total = np.zeros(3, np.float64)
    count = 0
    for e in estimates:
        if isinstance(e, tuple) and len(e) == 2:
            e = e[1]
        total += np.asarray(e, dtype=np.float64).reshape(3)
        count += 1
    if count == 0:
        raise ValueError("balance_from needs at least one estimate")
    return beta_from_sums(total)


def pair_range(n, f_lo=None, f_hi=None):
    """(m_lo, m_hi), inclusive: the mirror pairs of an n-bin spectrum whose upper member lies in [f_lo, f_hi) Hz above the
    input frequency -- rounded as ``spectrum.span_bins`` rounds a span, None being the first pair (1) and the end of the
    pairs (floor((n - 1) / 2) inclusive).  ValueError for an empty range or one that leaves the pairs."""
    n = int(n)
    last = (n - 1) // 2
    m_lo = 1 if f_lo is None else int(round(float(f_lo)))
    m_hi = last if f_hi is None else int(round(float(f_hi))) - 1
    if m_hi < m_lo:
        raise ValueError("empty range of mirror pairs: f_hi must lie above f_lo (and n must be at least 3)")
    if m_lo < 1 or m_hi > last:
        raise ValueError("pairs [%d, %d] leave the mirror pairs [1, %d] of a %d-bin spectrum" % (m_lo, m_hi, last, n))
    return m_lo, m_hi


def device_pairs(samples):
    """(flat contiguous device tensor of 2 N integers, RCFM_IQ_* format, N) of a numpy array or torch tensor shaped
    [N, 2] or [2 N]; ValueError for another dtype or shape, or an odd element count."""
    t = hip.torch()
    if isinstance(samples, t.Tensor):
        dt = {t.int16: np.dtype("int16"), t.int8: np.dtype("int8"), t.uint8: np.dtype("uint8")}.get(samples.dtype)
    else:
        samples = np.asarray(samples)
        dt = samples.dtype
    fmt = FORMATS.get(dt)
    if fmt is None:
        raise ValueError("raw IQ is int16, int8 or uint8, not %s" % (samples.dtype,))
    shape = tuple(samples.shape)
    if not (len(shape) == 1 or (len(shape) == 2 and shape[1] == 2)):
        raise ValueError("raw IQ is shaped [N, 2] or [2 N], not %s" % (list(shape),))
    if len(shape) == 1 and shape[0] % 2:
        raise ValueError("raw IQ holds I, Q pairs: an odd element count (%d)" % shape[0])
    x = hip.to_device(samples).reshape(-1)
    return x, fmt, int(x.shape[0]) // 2


def to_complex64(raw):
    """complex64 [N] device tensor of the raw buffer `raw` ([N, 2] or [2 N] int16 / int8 / uint8, host or device):
    rcfm_iq_convert on the current stream."""
    x, fmt, n = device_pairs(raw)
    out = hip.empty((n,), hip.torch().complex64)
    hip.check(hip.lib().rcfm_iq_convert(fmt, ctypes.c_size_t(n), hip.ptr(x), hip.ptr(out), hip.stream()))
    return out
