// The spectrum rules of the library, each written once: what scipy.signal.resample and scipy.signal.hilbert do to a
// bin, how two real signals come out of one complex FFT, which source bin a channel bin is gathered from.
// Scalars and float2 only -- no memory access, no device intrinsic -- so a host program can call every function
// (tests/spectrum_rules_host.hip, held against scipy itself by tests/test_spectrum_rules.py).  Each keeps the expression
// form of the hot kernels that use it: their machine code does not move.  Realised elsewhere, by ADDING the two Nyquist
// rows of a full spectrum instead of weighting a bin of a folded one (another operation on another layout), is
// resample_nyquist's factor 2: the decimating tiles (fft_decim_rt.h, fft_kernel.h) and lds_chain.hip (xs[A/2] += xs[A]).
#pragma once

#include <hip/hip_vector_types.h>

#define RCFM_RULE __host__ __device__ __forceinline__
#define RCFM_RULE_T template <typename I> RCFM_RULE   // I: the caller's index type (int, int64_t)

namespace rcfm {

// scipy.signal.resample's Nyquist bin when min(n, m) is even (scipy 1.15.3 _signaltools.py, "Split/join Nyquist component(s)")
enum NyquistMode : int { NYQ_NONE = 0, NYQ_DOWN = 1, NYQ_UP = 2 };

// scipy.signal.hilbert (pll.py:34): the mask h = {1, 2, ..., 2, (1), 0, ...} of length n at bin k, times `unit`;
// _low: 0 <= k < n / 2 is known.
RCFM_RULE_T float hilbert_weight_low(I k, float unit) { return (k == 0) ? unit : 2.f * unit; }
RCFM_RULE_T float hilbert_weight(I n, I k, float unit) {
    float h = hilbert_weight_low(k, unit);
    if (k >= (n + 1) / 2) h = 0.f;
    if ((n & 1) == 0 && k == n / 2) h = unit;
    return h;
}

// Bin k of a Hermitian spectrum of length m: kk = |k|, and whether bin k is the conjugate of bin kk.
template <typename I> struct Folded { I kk; bool mirrored; };
RCFM_RULE_T Folded<I> fold(I k, I m) { return Folded<I>{k > m / 2 ? m - k : k, k > m / 2}; }

// scipy.signal.resample of a real signal, n -> m (decimate.py:48): bin min(n, m) / 2, where min(n, m) is even, is
// doubled for m < n and halved for n < m (nyq_bin = -1: no such bin, or m == n where it is left alone) ...
RCFM_RULE int resample_nyquist_bin(long long n, long long m) {
    const long long nmin = n < m ? n : m;
    return ((nmin & 1) == 0 && m != n) ? (int)(nmin / 2) : -1;
}
RCFM_RULE float resample_nyquist_factor(long long n, long long m) { return resample_nyquist_bin(n, m) < 0 ? 1.f : (m < n ? 2.f : 0.5f); }
RCFM_RULE_T float resample_nyquist(float w, I kk, int nyq_bin, float nyq_factor) { return kk == nyq_bin ? w * nyq_factor : w; }
RCFM_RULE_T float2 resample_nyquist(float2 y, I kk, int nyq_bin, float nyq_factor) {
    return kk == nyq_bin ? make_float2(y.x * nyq_factor, y.y * nyq_factor) : y;
}
// ... and a real inverse transform of length m never sees the imaginary part of DC / Nyquist (pocketfft's c2r drops it).
RCFM_RULE_T bool real_bin_is_real(I kk, I m) { return kk == 0 || ((m & 1) == 0 && kk == m / 2); }

// Two real signals per complex FFT, U = FFT(x0 + j x1), a = U[k], b = U[-k]:
RCFM_RULE float2 pair_even(float2 a, float2 b) { return make_float2(a.x + b.x, a.y - b.y); }      // 2 X0[k] = U[k] + conj U[-k]
RCFM_RULE float2 pair_odd(float2 a, float2 b) { return make_float2(a.y + b.y, -(a.x - b.x)); }   // 2 X1[k] = (U[k] - conj U[-k]) / j

// wbfm.py:86-87 with decimate.py:48: point f of the packed Hermitian pair V = HL + j HR (ifft(V) = l + j r) of length m
// from a = U[kk], b = U[-kk] of U = FFT(l + j r) and the weight w of bin kk; live: kk lies inside the kept band.
RCFM_RULE_T float2 stereo_unpack_point(float2 a, float2 b, float w, Folded<I> f, bool live, int nyq_bin, float nyq_factor, I m) {
    float2 hl = make_float2(0.f, 0.f), hr = hl;   // (the products reach the sums below through this select: no FMA forms)
    if (live) {
        w = resample_nyquist(w, f.kk, nyq_bin, nyq_factor);
        const float2 e = pair_even(a, b), o = pair_odd(a, b);
        hl = make_float2(0.5f * e.x * w, 0.5f * e.y * w);
        hr = make_float2(0.5f * o.x * w, 0.5f * o.y * w);
        if (real_bin_is_real(f.kk, m)) hl.y = hr.y = 0.f;
    }
    if (f.mirrored) hl.y = -hl.y, hr.y = -hr.y;
    return make_float2(hl.x - hr.y, hl.y + hr.x);
}

// The channel gather, np.roll + truncate / zero-pad of a complex spectrum to B bins (tuner.py:159): signed offset of the
// source bin of channel bin k.  The plain form, every bin has a source (B <= N, no NYQ_UP) -- once for a run-time and once
// for a compile-time B: the compiler rewrites the select of a variable B before it inlines, the LDS chain's (constant B) not.
RCFM_RULE int gather_offset(int k, int B, int nyq) { return k < nyq ? k : k - B; }
template <int B> RCFM_RULE int gather_offset(int k, int nyq) { return k < nyq ? k : k - B; }
// The general form, branch-free per lane: ok = false is a zero-filled bin; NYQ_UP copies Y[-n/2] from Y[+n/2], both halved.
RCFM_RULE_T I gather_offset(I k, I B, int nyq, int nneg, int nyq_mode, bool& ok) {
    const I j = B - k;
    const bool pos = k < nyq;
    I d = pos ? k : -j;
    ok = pos | (j <= nneg);
    if (nyq_mode == NYQ_UP) {
        const bool up = !ok & (j == nyq - 1);
        d = up ? nyq - 1 : d;
        ok |= up;
    }
    return ok ? d : 0;
}
RCFM_RULE_T bool nyquist_up_halved(I k, I B, int nyq) { return k == nyq - 1 || (B - k) == nyq - 1; }

// Single sideband, s = Re(ifft(H X)) resampled as a real signal: bins 1 .. kmax survive (DC and the bin n / 2 are dropped);
// weights (of Re, of Im) of bin kk given its weight w: conj for LSB, conj again when mirrored, a real Nyquist bin.
RCFM_RULE_T bool ssb_kept(I kk, int kmax) { return kk >= 1 && kk <= kmax; }
RCFM_RULE_T float2 ssb_weights(float w, I kk, int kmax, bool mirrored, bool lower, int nyq_bin, float nyq_factor) {
    if (!ssb_kept(kk, kmax)) w = 0.f;
    if (kk == nyq_bin) w *= nyq_factor;
    return make_float2(w, (kk == nyq_bin) ? 0.f : (lower != mirrored ? -w : w));
}

// WBFM's same-size Decimate (decimate.py:48 with m == n): a three-tap circular Hamming filter.
RCFM_RULE float hamming3(float l, float c, float r, float side_tap) { return 0.54f * c + side_tap * (l + r); }

}  // namespace rcfm
