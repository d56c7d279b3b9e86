"""csrc/spectrum_rules.h on the host: tests/spectrum_rules_host.hip prints what each rule returns, and the table is
held against scipy itself (resample, hilbert), numpy's FFT (pair unpack) and index arithmetic in numpy.fft.fftfreq
ordering (fold, gather offsets, single sideband).  No GPU: the header has no memory access and no device intrinsic.

The reference's own rules, written in numpy, meet the two scipy bounds at 4.4e-16 and 5.0e-16 (scipy 1.15.3)."""

import os
import subprocess

import numpy as np
import pytest
import scipy.signal

from conftest import ROOT

CSRC = os.path.join(ROOT, "radio-core_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "spectrum_rules_host.hip")
TOL = 1e-12
NONE, DOWN, UP = 0, 1, 2

RESAMPLE = [(n, m) for n in (2, 3, 7, 8, 9, 10) for m in (2, 3, 5, 6, 7, 8, 9, 10, 12)]
HILBERT = (1, 2, 3, 4, 7, 8)
PAIR = (1, 2, 5, 8)
GATHER_B = (2, 3, 8, 9)
GATHER_N = (2, 3, 4, 6, 8, 9, 16, 18)          # source lengths: shorter than, equal to and longer than every B
SSB = [(a, b) for a in (2, 3, 8, 9) for b in (3, 4, 8, 9, 16)]


def _hipcc():
    for line in open(os.path.join(ROOT, "radio-core_amd", "Makefile")):
        if line.startswith("HIPCC"):
            return os.environ.get("HIPCC", line.split("?=")[1].strip())
    raise AssertionError("the Makefile names no compiler")


def _bins(u):
    return " ".join("%.9g %.9g" % (v.real, v.imag) for v in u)


def _pair_spectrum(n, seed):
    """U with small integer parts (exact in float32, as are the members' sums), and the x0, x1 it is the FFT of."""
    rng = np.random.default_rng(seed)
    u = rng.integers(-8, 9, n) + 1j * rng.integers(-8, 9, n)
    x = np.fft.ifft(u)
    assert np.max(np.abs(np.fft.fft(x.real + 1j * x.imag) - u)) <= TOL
    return u, x.real, x.imag


def _resample_geom(n, m):
    """scipy.signal.resample's slices for complex input n -> m: positive bins, negative bins, Nyquist mode."""
    nmin = min(n, m)
    nyq = nmin // 2 + 1
    nneg = nmin - nyq if nmin > 2 else 0
    mode = NONE
    if nmin % 2 == 0 and m < n and nmin > 2:
        mode = DOWN
    elif nmin % 2 == 0 and n < m:
        mode = UP
    return nyq, nneg, mode


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rules") / "spectrum_rules_host")
    subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                   check=True)
    req = ["H %d" % n for n in HILBERT] + ["R %d %d" % nm for nm in RESAMPLE] + ["F %d" % m for m in range(1, 11)]
    for n in PAIR:
        req.append("P %d %s" % (n, _bins(_pair_spectrum(n, n)[0])))
    for n, m in RESAMPLE:
        req.append("U %d %d %s" % (n, m, _bins(_pair_spectrum(n, 100 + n)[0])))
    for B in GATHER_B:
        for n in GATHER_N:
            nyq, nneg, _ = _resample_geom(n, B)
            req += ["G %d %d %d %d" % (B, nyq, nneg, mode) for mode in (NONE, DOWN, UP)]
    for a, b in SSB:
        kmax = min(a // 2, (b - 1) // 2)
        for lower in (0, 1):
            req.append("S %d %d %d %.9g %d" % (a, kmax, _nyq_bin(b, a), _nyq_factor(b, a), lower))
    req = list(dict.fromkeys(req))   # (several source lengths share one gather or sideband geometry)
    out = subprocess.run([exe], input="\n".join(req) + "\n", check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        f = line.split()
        rows.setdefault(f[0], []).append(f[1:])
    return rows


def _nyq_bin(n, m):
    return min(n, m) // 2 if min(n, m) % 2 == 0 and n != m else -1


def _nyq_factor(n, m):
    return 1.0 if _nyq_bin(n, m) < 0 else (2.0 if m < n else 0.5)


def _select(rows, *key):
    key = [str(k) for k in key]
    return [r[len(key):] for r in rows if r[:len(key)] == key]


@pytest.mark.parametrize("n,m", RESAMPLE)
def test_resample_rule_is_scipys(table, n, m):
    x = np.random.default_rng(1000 * n + m).standard_normal(n)
    rows = _select(table["R"], n, m)
    head, rows = rows[0], rows[1:]
    assert head[0] == "bin" and int(head[1]) == _nyq_bin(n, m) and float(head[2]) == _nyq_factor(n, m)
    assert [int(r[0]) for r in rows] == list(range(m // 2 + 1))
    factor = np.array([float(r[1]) for r in rows])
    assert [float(r[2]) for r in rows] == list(factor)                       # the float2 form scales both parts alike
    real = np.array([int(r[3]) for r in rows], bool)
    X = np.fft.rfft(x)
    Y = np.zeros(m // 2 + 1, complex)
    nyq = min(n, m) // 2 + 1
    Y[:nyq] = X[:nyq] * factor[:nyq]
    # a bin the rule calls real is one whose imaginary part the inverse transform must not see: poison it
    Y.imag[real] = 0.0
    poisoned = Y.copy()
    poisoned.imag[real] = 1e3
    want = scipy.signal.resample(x, m)
    assert np.max(np.abs(np.fft.irfft(Y, m) * (m / n) - want)) <= TOL
    assert np.max(np.abs(np.fft.irfft(poisoned, m) * (m / n) - want)) <= TOL      # exactly the bins irfft ignores
    assert list(np.flatnonzero(real)) == [0] + ([m // 2] if m % 2 == 0 else [])


@pytest.mark.parametrize("n", HILBERT)
def test_hilbert_mask_is_scipys(table, n):
    x = np.random.default_rng(n).standard_normal(n)
    rows = _select(table["H"], n)
    assert [int(r[0]) for r in rows] == list(range(n))
    h = np.array([float(r[1]) for r in rows])
    assert np.max(np.abs(np.fft.ifft(np.fft.fft(x) * h) - scipy.signal.hilbert(x))) <= TOL


@pytest.mark.parametrize("n", PAIR)
def test_pair_members_are_the_two_transforms(table, n):
    _, x0, x1 = _pair_spectrum(n, n)
    rows = np.array(_select(table["P"], n), float)
    assert list(rows[:, 0]) == list(range(n))
    assert np.max(np.abs(rows[:, 1] + 1j * rows[:, 2] - np.fft.fft(x0))) <= TOL
    assert np.max(np.abs(rows[:, 3] + 1j * rows[:, 4] - np.fft.fft(x1))) <= TOL


@pytest.mark.parametrize("n,m", RESAMPLE)
def test_stereo_unpack_point_resamples_both_members(table, n, m):
    """The shared combine of k_stereo_unpack and LoadStereoUnpack: ifft of the packed pair is resample(x0) + j resample(x1)."""
    _, x0, x1 = _pair_spectrum(n, 100 + n)
    rows = np.array(_select(table["U"], n, m), float)
    assert list(rows[:, 0]) == list(range(m))
    got = np.fft.ifft(rows[:, 1] + 1j * rows[:, 2]) * (m / n)
    want = scipy.signal.resample(x0, m) + 1j * scipy.signal.resample(x1, m)
    # the spectrum reached the program in float32 with integer parts, exactly; its sums are exact too, and the
    # factors are powers of two: what is left is float64 rounding of the two inverse transforms
    assert np.max(np.abs(got - want)) <= TOL


@pytest.mark.parametrize("m", range(1, 11))
def test_fold_is_the_signed_frequency(table, m):
    s = np.rint(np.fft.fftfreq(m) * m).astype(int)
    rows = np.array(_select(table["F"], m), int)
    assert list(rows[:, 0]) == list(range(m))
    assert list(rows[:, 1]) == list(np.abs(s))
    # bin m / 2 of an even length is its own conjugate: it counts as not mirrored
    assert list(rows[:, 2]) == [int(v < 0 and 2 * -v != m) for v in s]


@pytest.mark.parametrize("B", GATHER_B)
@pytest.mark.parametrize("mode", (NONE, DOWN, UP))
def test_gather_offsets(table, B, mode):
    s = np.rint(np.fft.fftfreq(B) * B).astype(int)
    for n in GATHER_N:
        nyq, nneg, _ = _resample_geom(n, B)
        rows = np.array(_select(table["G"], B, nyq, nneg, mode), int)
        assert list(rows[:, 0]) == list(range(B))
        half = nyq - 1
        for k in range(B):
            # scipy copies X[0 : nyq] and X[-nneg :]: output bin k holds frequency +k where k < nyq, else k - B
            f = k if k < nyq else k - B
            ok = f >= -nneg
            d = f if ok else 0
            if mode == UP and not ok and f == -half:       # Y[-N/2] = Y[+N/2]
                ok, d = True, half
            assert (rows[k, 1], rows[k, 2]) == (d, int(ok)), (B, n, mode, k)
            assert rows[k, 3] == int(abs(f) == half or k == half), (B, n, mode, k)
            if B <= n and mode != UP:                       # the plain form: every bin has a source
                assert ok and rows[k, 4] == d, (B, n, k)
                if nyq == B // 2 + 1:                       # ... the signed frequency, bin B / 2 counted as +B / 2
                    assert d == (s[k] if 2 * k != B else k)


@pytest.mark.parametrize("a,b", SSB)
@pytest.mark.parametrize("lower", (0, 1))
def test_ssb_rule(table, a, b, lower):
    kmax = min(a // 2, (b - 1) // 2)
    rows = _select(table["S"], a, kmax, _nyq_bin(b, a), lower)
    s = np.rint(np.fft.fftfreq(a) * a).astype(int)
    want = []
    for k in range(a):
        f = abs(s[k])
        kept = 1 <= f <= kmax
        nyq = f == _nyq_bin(b, a)
        w = (1.0 if kept else 0.0) * (_nyq_factor(b, a) if nyq else 1.0)
        # the functor multiplies X[+f] (USB) or X[-f] (LSB) part by part: conj for LSB, conj again for negative k
        conj = bool(lower) != (s[k] < 0 and 2 * f != a)
        want.append((k, int(kept), w, 0.0 if nyq else (-w if conj else w)))
    assert [(int(r[0]), int(r[1]), float(r[2]), float(r[3])) for r in rows] == want
