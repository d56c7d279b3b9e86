// IQ imbalance estimate and image rejection on the loaded spectrum (include/rcfm.h, "IQ balance"): rcfm_tuner_iq_estimate,
// rcfm_tuner_iq_correct, rcfm_tuner_set_iq_balance.  A receiver whose I and Q paths differ in gain and phase delivers
// x' = mu x + nu conj(x); in the spectrum bin k then carries nu conj(X[-k]), the image of its mirror bin.  Both passes
// stream over the spectrum once, each thread holding mirror pairs (m, n - m): one side ascends, the other descends.

#include "iq_balance.h"

#include <cmath>

#include "api_internal.h"

namespace rcfm {

namespace {

// Re P, Im P, Q of the pairs a thread, a wave, a workgroup has seen.
struct IqAcc {
    double pr, pi, q;
};

// One mirror pair: P += a b (no conjugate), Q += |a|^2 + |b|^2.  Every product of two float32 is exact in float64.
__device__ __forceinline__ void iq_term(IqAcc& s, float2 a, float2 b) {
    const double ar = a.x, ai = a.y, br = b.x, bi = b.y;
    s.pr += ar * br - ai * bi;
    s.pi += ar * bi + ai * br;
    s.q += (ar * ar + ai * ai) + (br * br + bi * bi);
}

// Segment blockIdx.x of gridDim.x = iq_segments(pairs) (iq_balance.h).  The pairs from the first even m on are taken two
// at a time, a "duo" (m, m + 1): X[m], X[m + 1] ascending and X[n - m - 1], X[n - m] descending -- lane i of a wave reads
// 16 bytes at X + m + 2 i and 16 bytes at X + n - m - 1 - 2 i, both one contiguous block per wave.  The duos are split
// evenly over the segments; thread 0 of segment 0 adds the pair in front of the first duo (m_lo odd) and the one behind the
// last.  VEC_A: X is 16-byte aligned, so X + m (m even) is one 16-byte load.  VEC_D: n is odd as well, so X + n - m - 1 is
// too; for even n that address is 8 bytes off and the descending side takes two 8-byte loads.  The loads differ, the
// order of the sums does not: per-thread strided float64, the waves' shuffle tree, the wave sums in order.
template <bool VEC_A, bool VEC_D>
__global__ __launch_bounds__(kIqBalThreads) void k_iq_estimate(const float2* __restrict__ X, int64_t n, int64_t m_lo,
                                                               int64_t m_hi, double* __restrict__ part) {
    __shared__ double red[3][kIqBalThreads / 64];
    const int seg = blockIdx.x, segs = gridDim.x, tid = threadIdx.x;
    const int64_t m0 = m_lo + (m_lo & 1);
    const int64_t rest = m_hi + 1 - m0;   // pairs from m0 on (0 when the range is the one odd pair m_lo)
    const int64_t duos = rest / 2;
    const int64_t per = (duos + segs - 1) / segs;
    const int64_t q1 = (int64_t)(seg + 1) * per < duos ? (int64_t)(seg + 1) * per : duos;
    IqAcc acc{0.0, 0.0, 0.0};
    for (int64_t q = (int64_t)seg * per + tid; q < q1; q += kIqBalThreads) {
        const int64_t m = m0 + 2 * q;
        float2 a0, a1, b0, b1;   // X[m], X[m + 1], X[n - m], X[n - m - 1]
        if (VEC_A) {
            const float4 v = *reinterpret_cast<const float4*>(X + m);
            a0 = make_float2(v.x, v.y);
            a1 = make_float2(v.z, v.w);
        } else {
            a0 = X[m];
            a1 = X[m + 1];
        }
        if (VEC_D) {
            const float4 v = *reinterpret_cast<const float4*>(X + (n - m - 1));
            b1 = make_float2(v.x, v.y);
            b0 = make_float2(v.z, v.w);
        } else {
            b1 = X[n - m - 1];
            b0 = X[n - m];
        }
        iq_term(acc, a0, b0);
        iq_term(acc, a1, b1);
    }
    if (seg == 0 && tid == 0) {
        if (m_lo & 1) iq_term(acc, X[m_lo], X[n - m_lo]);
        if (rest & 1) iq_term(acc, X[m_hi], X[n - m_hi]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        acc.pr += __shfl_down(acc.pr, off, 64);
        acc.pi += __shfl_down(acc.pi, off, 64);
        acc.q += __shfl_down(acc.q, off, 64);
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = acc.pr;
        red[1][tid >> 6] = acc.pi;
        red[2][tid >> 6] = acc.q;
    }
    __syncthreads();
    if (tid != 0) return;
    double tot[3] = {0.0, 0.0, 0.0};
    for (int w = 0; w < kIqBalThreads / 64; ++w)
        for (int j = 0; j < 3; ++j) tot[j] += red[j][w];
    for (int j = 0; j < 3; ++j) part[3 * (int64_t)seg + j] = tot[j];
}

// One workgroup; ONE thread adds: the segments' sums in segment order, then c = 2 P / Q and
// beta = c / (1 + sqrt(1 - min(|c|^2, 1))), the inverse of c = 2 beta / (1 + |beta|^2), in float64 without contraction and
// rounded to float32 once.  Q = 0 or anything non-finite: beta = 0.  The other threads only fetch: a single thread walking
// 3 x 1024 partial sums in global memory has one wave's worth of loads in flight and took longer than the estimate of the
// airband spectrum itself, so the workgroup stages them in LDS (24 KiB) with coalesced loads first.
__global__ __launch_bounds__(kIqBalThreads) void k_iq_finish(const double* __restrict__ part, int segs,
                                                             double* __restrict__ sums, float* __restrict__ beta) {
#pragma clang fp contract(off)
    __shared__ double staged[3 * kIqMaxSegs];
    for (int i = threadIdx.x; i < 3 * segs; i += kIqBalThreads) staged[i] = part[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double pr = 0.0, pi = 0.0, q = 0.0;
    for (int s = 0; s < segs; ++s) {
        pr += staged[3 * s];
        pi += staged[3 * s + 1];
        q += staged[3 * s + 2];
    }
    if (sums) {
        sums[0] = pr;
        sums[1] = pi;
        sums[2] = q;
    }
    if (!beta) return;
    double br = 0.0, bi = 0.0;
    if (q > 0.0 && isfinite(pr) && isfinite(pi) && isfinite(q)) {
        const double cr = (2.0 * pr) / q, ci = (2.0 * pi) / q;
        const double c2 = fmin(cr * cr + ci * ci, 1.0);
        const double d = 1.0 + sqrt(1.0 - c2);
        br = cr / d;
        bi = ci / d;
        if (!(isfinite(br) && isfinite(bi))) br = bi = 0.0;
    }
    beta[0] = (float)br;
    beta[1] = (float)bi;
}

// a - beta conj(b) in float32: at most three roundings per component.
__device__ __forceinline__ float2 iq_fix(float2 a, float2 b, float br, float bi) {
    return make_float2(a.x - (br * b.x + bi * b.y), a.y - (bi * b.x - br * b.y));
}

// The halo copies of the pair (m, n - m), 1 <= m < n - m: bins [0, halo) repeat behind bin n - 1, bins [n - halo, n) in
// front of bin 0.
__device__ __forceinline__ void iq_halo_pair(float2* __restrict__ X, int64_t n, int64_t halo, int64_t m, float2 ya, float2 yb) {
    if (m < halo) X[n + m] = ya;
    if (m <= halo) X[-m] = yb;
}

// Slot m of 0 .. floor(n / 2), the general form: bin m and its mirror, or bin m alone where it is its own mirror (m = 0,
// and m = n / 2 for even n), with the notch and the halo copies.
__device__ __forceinline__ void iq_correct_slot(float2* __restrict__ X, int64_t n, int64_t halo, int64_t m, int64_t notch,
                                                float br, float bi) {
    const float2 zero = make_float2(0.f, 0.f);
    if (m == 0 || 2 * m == n) {
        const float2 a = X[m];
        const float2 y = m < notch ? zero : iq_fix(a, a, br, bi);
        X[m] = y;
        if (m == 0 && halo > 0) X[n] = y;
        if (m != 0 && halo >= m) X[m - n] = y;   // (halo = n / 2: the front halo starts with bin n / 2)
        return;
    }
    const float2 a = X[m], b = X[n - m];
    const float2 ya = m < notch ? zero : iq_fix(a, b, br, bi), yb = m < notch ? zero : iq_fix(b, a, br, bi);
    X[m] = ya;
    X[n - m] = yb;
    iq_halo_pair(X, n, halo, m, ya, yb);
}

// Y[k] = X[k] - beta conj(X[(n - k) mod n]) in place (iq_balance.h, launch_iq_correct).  Thread q owns slots 2 q and
// 2 q + 1 of 0 .. floor(n / 2): it reads both members of each pair before it writes either, nobody else touches them, and
// it writes their halo copies too (the halos are never read).  Where both slots are plain pairs the loads and stores are
// those of k_iq_estimate (VEC_A, VEC_D); the duo with bin 0 and the last one, which may hold bin n / 2 or a single slot,
// take the general form.
template <bool VEC_A, bool VEC_D>
__global__ __launch_bounds__(kIqBalThreads) void k_iq_correct(float2* __restrict__ X, int64_t n, int64_t halo,
                                                              const float* __restrict__ beta, int64_t notch) {
    const float br = beta[0], bi = beta[1];
    const int64_t hm = n / 2, duos = hm / 2 + 1;
    const int64_t stride = (int64_t)gridDim.x * kIqBalThreads;
    for (int64_t q = (int64_t)blockIdx.x * kIqBalThreads + threadIdx.x; q < duos; q += stride) {
        const int64_t m = 2 * q;
        if (q == 0 || 2 * (m + 1) >= n) {
            iq_correct_slot(X, n, halo, m, notch, br, bi);
            if (m + 1 <= hm) iq_correct_slot(X, n, halo, m + 1, notch, br, bi);
            continue;
        }
        float2 a0, a1, b0, b1;   // X[m], X[m + 1], X[n - m], X[n - m - 1]
        if (VEC_A) {
            const float4 v = *reinterpret_cast<const float4*>(X + m);
            a0 = make_float2(v.x, v.y);
            a1 = make_float2(v.z, v.w);
        } else {
            a0 = X[m];
            a1 = X[m + 1];
        }
        if (VEC_D) {
            const float4 v = *reinterpret_cast<const float4*>(X + (n - m - 1));
            b1 = make_float2(v.x, v.y);
            b0 = make_float2(v.z, v.w);
        } else {
            b1 = X[n - m - 1];
            b0 = X[n - m];
        }
        const float2 zero = make_float2(0.f, 0.f);
        const float2 ya0 = m < notch ? zero : iq_fix(a0, b0, br, bi), yb0 = m < notch ? zero : iq_fix(b0, a0, br, bi);
        const float2 ya1 = m + 1 < notch ? zero : iq_fix(a1, b1, br, bi), yb1 = m + 1 < notch ? zero : iq_fix(b1, a1, br, bi);
        if (VEC_A) {
            *reinterpret_cast<float4*>(X + m) = make_float4(ya0.x, ya0.y, ya1.x, ya1.y);
        } else {
            X[m] = ya0;
            X[m + 1] = ya1;
        }
        if (VEC_D) {
            *reinterpret_cast<float4*>(X + (n - m - 1)) = make_float4(yb1.x, yb1.y, yb0.x, yb0.y);
        } else {
            X[n - m - 1] = yb1;
            X[n - m] = yb0;
        }
        if (m <= halo) {
            iq_halo_pair(X, n, halo, m, ya0, yb0);
            iq_halo_pair(X, n, halo, m + 1, ya1, yb1);
        }
    }
}

}  // namespace

void launch_iq_estimate(const float2* X, int64_t n, int64_t m_lo, int64_t m_hi, double* part, double* sums, float* beta,
                        hipStream_t stream) {
    const int segs = iq_segments(m_hi - m_lo + 1);
    const bool vec_a = (uintptr_t)X % 16 == 0, vec_d = vec_a && (n & 1);
    const dim3 grid((unsigned)segs), block(kIqBalThreads);
    if (vec_d) hipLaunchKernelGGL((k_iq_estimate<true, true>), grid, block, 0, stream, X, n, m_lo, m_hi, part);
    else if (vec_a) hipLaunchKernelGGL((k_iq_estimate<true, false>), grid, block, 0, stream, X, n, m_lo, m_hi, part);
    else hipLaunchKernelGGL((k_iq_estimate<false, false>), grid, block, 0, stream, X, n, m_lo, m_hi, part);
    RC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_iq_finish, dim3(1), dim3(kIqBalThreads), 0, stream, part, segs, sums, beta);
    RC_HIP(hipGetLastError());
}

void launch_iq_correct(float2* X, int64_t n, int64_t halo, const float* beta, int64_t notch, hipStream_t stream) {
    const int64_t duos = (n / 2) / 2 + 1;
    const bool vec_a = (uintptr_t)X % 16 == 0, vec_d = vec_a && (n & 1);
    const dim3 grid((unsigned)std::min<int64_t>((duos + kIqBalThreads - 1) / kIqBalThreads, kIqCorrectBlocks)), block(kIqBalThreads);
    if (vec_d) hipLaunchKernelGGL((k_iq_correct<true, true>), grid, block, 0, stream, X, n, halo, beta, notch);
    else if (vec_a) hipLaunchKernelGGL((k_iq_correct<true, false>), grid, block, 0, stream, X, n, halo, beta, notch);
    else hipLaunchKernelGGL((k_iq_correct<false, false>), grid, block, 0, stream, X, n, halo, beta, notch);
    RC_HIP(hipGetLastError());
}

}  // namespace rcfm

using namespace rcfm;

// Every bin of the spectrum is held on this device: a plain load, into the handle's own storage or an attached one.
void rcfm_tuner_s::require_whole(const char* caller) const {
    RC_REQUIRE(loaded, RCFM_ERR_STATE, std::string(caller) + " called before rcfm_tuner_load");
    RC_REQUIRE(!ext_window && !loaded_windowed && held_bins >= n, RCFM_ERR_STATE,
               std::string(caller) + " needs every bin and its mirror: the loaded, sharded or attached spectrum holds a window only");
}

void rcfm_tuner_s::iq_estimate(int64_t m_lo, int64_t m_hi, double* sums, float* beta, hipStream_t s) {
    require_whole("rcfm_tuner_iq_estimate");
    iq_part.reserve(sizeof(double) * 3 * (size_t)iq_segments(m_hi - m_lo + 1));
    launch_iq_estimate(spectrum(), n, m_lo, m_hi, iq_part.as<double>(), sums, beta, s);
}

void rcfm_tuner_s::iq_correct(const float* beta, int64_t notch, hipStream_t s) {
    require_whole("rcfm_tuner_iq_correct");
    launch_iq_correct(spectrum(), n, halo, beta, notch, s);
}

// What rcfm_tuner_load and rcfm_tuner_load_raw queue behind the FFT (rcfm_tuner_set_iq_balance): nothing when off.
void rcfm_tuner_s::iq_after_load(hipStream_t s) {
    if (iq_mode == RCFM_IQ_BALANCE_OFF) return;
    if (iq_mode == RCFM_IQ_BALANCE_AUTO) iq_estimate(1, (n - 1) / 2, nullptr, iq_beta_auto.as<float>(), s);
    iq_correct(iq_mode == RCFM_IQ_BALANCE_AUTO ? iq_beta_auto.as<float>() : iq_beta_fixed.as<float>(), iq_notch, s);
}

extern "C" {

int rcfm_tuner_iq_estimate(rcfm_tuner_t t, int64_t m_lo, int64_t m_hi, void* sums, void* beta, void* stream) {
    return guarded([&] {
        RC_REQUIRE(sums || beta, RCFM_ERR_ARG, "both outputs are NULL");
        RC_REQUIRE(m_lo >= 1 && m_hi >= m_lo, RCFM_ERR_ARG, "empty pair range: 1 <= m_lo <= m_hi");
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(m_hi <= (t->n - 1) / 2, RCFM_ERR_ARG, "the pair range leaves the mirror pairs 1 .. floor((n - 1) / 2)");
        ArenaScope scope(t->arena);
        t->iq_estimate(m_lo, m_hi, static_cast<double*>(sums), static_cast<float*>(beta), as_stream(stream));
    });
}

int rcfm_tuner_iq_correct(rcfm_tuner_t t, const void* beta, int64_t dc_notch, void* stream) {
    return guarded([&] {
        RC_REQUIRE(beta != nullptr, RCFM_ERR_ARG, "beta is NULL");
        RC_REQUIRE(dc_notch >= 0, RCFM_ERR_ARG, "negative dc_notch");
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(dc_notch <= t->n / 2, RCFM_ERR_ARG, "dc_notch exceeds n / 2");
        ArenaScope scope(t->arena);
        t->iq_correct(static_cast<const float*>(beta), dc_notch, as_stream(stream));
    });
}

int rcfm_tuner_set_iq_balance(rcfm_tuner_t t, int mode, float beta_re, float beta_im, int64_t dc_notch) {
    return guarded([&] {
        RC_REQUIRE(mode == RCFM_IQ_BALANCE_OFF || mode == RCFM_IQ_BALANCE_FIXED || mode == RCFM_IQ_BALANCE_AUTO, RCFM_ERR_ARG,
                   "unknown balance mode (RCFM_IQ_BALANCE_OFF, _FIXED, _AUTO)");
        RC_REQUIRE(dc_notch >= 0, RCFM_ERR_ARG, "negative dc_notch");
        if (mode == RCFM_IQ_BALANCE_FIXED) {
            RC_REQUIRE(std::isfinite(beta_re) && std::isfinite(beta_im), RCFM_ERR_ARG, "beta is not finite");
            RC_REQUIRE((double)beta_re * beta_re + (double)beta_im * beta_im < 1.0, RCFM_ERR_ARG, "|beta| must be below 1");
        }
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(dc_notch <= t->n / 2, RCFM_ERR_ARG, "dc_notch exceeds n / 2");
        RC_REQUIRE(mode != RCFM_IQ_BALANCE_AUTO || t->n >= 3, RCFM_ERR_ARG, "a spectrum of fewer than 3 bins has no mirror pairs to estimate from");
        if (mode == RCFM_IQ_BALANCE_FIXED) {
            const float b[2] = {beta_re, beta_im};
            t->iq_beta_fixed.upload(b, sizeof(b));
        }
        if (mode == RCFM_IQ_BALANCE_AUTO) t->iq_beta_auto.reserve(2 * sizeof(float));
        t->iq_mode = mode;
        t->iq_notch = dc_notch;
    });
}

}  // extern "C"
