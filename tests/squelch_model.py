"""Signal-level and squelch test model (no test functions): the definition of include/rcfm.h (rcfm_tuner_levels,
rcfm_squelch) from the oracle's own pieces, in float64.

    level[c] = sum_k |Y_c[k]|^2 / N^2,  Y_c = radiocore_oracle.tuner_channel_spectrum(X, N, roll_c, B_c)
which by Parseval is mean(|radiocore_oracle.Tuner.run_pruned(c)|^2); a channel is open iff level >= threshold.
"""

import numpy as np

import am_model


def level(oracle, X, n, roll, B):
    """Level of one channel (roll, bandwidth B <= n) of the n-point spectrum X."""
    Y = oracle.tuner_channel_spectrum(X, int(n), int(roll), int(B))
    return float(np.sum(Y.real ** 2 + Y.imag ** 2)) / float(n) ** 2


def levels(oracle, ref_tuner, first=0, count=None):
    """float64 [count]: the levels of channels [first, first + count) of a loaded radiocore_oracle.Tuner.  Load it with
    the buffer as complex128 (numpy transforms complex64 input in single precision): the expectation is float64."""
    count = len(ref_tuner.channels()) - first if count is None else count
    X = ref_tuner._buffer
    out = np.empty(count)
    for i in range(count):
        roll, B = ref_tuner._roll(first + i)
        out[i] = level(oracle, X, X.shape[0], roll, B)
    return out


def open_mask(lv, threshold):
    """The squelch rule: open iff level >= threshold (false for NaN on either side)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(lv, np.float64) >= np.asarray(threshold, np.float64)


def margin_db(lv, threshold):
    """How far the nearest level is from its threshold, in dB (inf when a level is 0)."""
    lv, threshold = np.asarray(lv, np.float64), np.broadcast_to(np.asarray(threshold, np.float64), np.shape(lv))
    with np.errstate(divide="ignore"):
        return float(np.min(np.abs(10.0 * np.log10(lv / threshold))))


def sparse_band(N, f_in, centres, B, planted, seed=0, noise=1e-4):
    """complex64 [N]: am_model.wideband with stations[i] on the channels of `planted` ({index: complex [B]}) and
    nothing but the wideband noise (standard deviation `noise` per component) on the others."""
    silent = np.zeros(B, np.complex128)

    def own_bins(x):
        # For even B the station's bin -B/2 is also bin +B/2 of the channel below (its Nyquist merge reads both): a
        # station that fills its channel would put that one bin into the neighbour, comparable to the noise floor.  The
        # planted stations carry nothing there, so an empty channel holds the wideband noise and nothing else.
        S = np.fft.fft(x)
        if B % 2 == 0:
            S[B // 2] = 0.0
        return np.fft.ifft(S)
    return am_model.wideband(N, f_in, centres, B, [own_bins(planted[i]) if i in planted else silent for i in range(len(centres))],
                             noise=noise, seed=seed)
