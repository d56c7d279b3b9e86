// Stateful AGC tail (include/rcfm.h, rcfm_agc / rcfm_demod_set_agc): one first-order follower per row, carried from
// call to call in one float of state, and the division by it.  Replaces k_am_tail / k_ssb_tail where a handle asks.

#include "agc.h"

#include <cmath>

#include "common.h"

namespace rcfm {

namespace {

constexpr int kWaves = kAgcThreads / 64;

__device__ __forceinline__ float clip999(float v) {
    return (v < -0.999f) ? -0.999f : ((v > 0.999f) ? 0.999f : v);   // NaN stays NaN like np.clip
}

// What the kernel takes: lambda and its powers from the host, in float64.
struct AgcArgs {
    double alpha;       // 1 - lambda, lambda = exp(-1 / decay_samples)
    double lambda;
    double kappa;       // log2(e) / decay_samples: lambda^k = exp2(-k kappa)
    double run_full;    // lambda^agc_run(kAgcSegment): what a whole run of a whole segment decays by
    double run_last;    // lambda^agc_run(n % kAgcSegment): the same for the row's last, shorter segment
    float level, floor;
};

// lambda^age = exp2(-age kappa), age >= 0.  The exponent is formed in float64 and split into a whole part (an exact
// power of two) and a fraction in [0, 1) for the hardware exponential: the relative error stays near 1e-7 whatever
// the age, where a float32 lambda multiplied in sample after sample drifts by 1e-3 over two seconds.
__device__ __forceinline__ float agc_decay(int age, double kappa) {
    const double e = fmin(fmax((double)age * kappa, 0.0), 300.0);
    const double whole = floor(e);
    return ldexpf(exp2f(-(float)(e - whole)), -(int)whole);
}

// PEAK: every sample is a candidate |v[k]| that decays at the one rate lambda, so which of two candidates is larger
// never changes with time and a prefix of the row is summed up by ONE of them: e[n] = p lambda^(n - pos).  Across runs,
// segments and calls the value is always evaluated from the sample itself -- no rounding accumulates along the row;
// inside a run of at most 33 samples the follower steps by lambda in float64.
struct Peak {
    float p;
    int pos;
};
__device__ __forceinline__ Peak peak_join(Peak a, Peak b, double kappa) {   // a lies before b
    return (a.p * agc_decay(b.pos - a.pos, kappa) >= b.p) ? a : b;
}

// CARRIER: c' = c + alpha (v - c) over a run is the affine map c -> d c + b.
struct Affine {
    double d, b;
};
__device__ __forceinline__ Affine affine_join(Affine a, Affine b) {   // a first, then b
    return Affine{a.d * b.d, fma(b.d, a.b, b.b)};
}

// Row blockIdx.x of v [batch][n] -> audio, follower state[blockIdx.x] in and out (agc.h).  The row goes through LDS in
// segments of kAgcSegment samples, one read and one write of memory per sample.  Per segment: every thread reduces its
// run of agc_run(len) samples to an aggregate; the 256 aggregates are scanned with wave shuffles and the four wave
// totals in order; a second sweep over the same LDS restarts each run from its carry, divides, clips and leaves the
// audio in LDS for a coalesced store.  The segment's total is the next segment's carry.
// VEC (n % 4 == 0, both rows 16-byte aligned): 16-byte loads and stores.
// CARRIER without history (state < 0) starts from the row's mean: thread t adds samples t, t + 256, ... in float64,
// the waves' shuffle tree, the four wave sums in order (as k_ssb_tail sums) -- from LDS when the row is one segment,
// else in a pass of its own over the row before anything is stored.
template <int MODE, bool VEC>
__global__ __launch_bounds__(kAgcThreads) void k_agc_tail(const float* v, float* audio, int64_t n, AgcArgs prm,
                                                          float* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) float buf[kAgcSegment];
    __shared__ double red[kWaves];
    __shared__ Peak wpeak[kWaves];
    __shared__ Affine waff[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* vr = v + (int64_t)blockIdx.x * n;
    float* ar = audio + (int64_t)blockIdx.x * n;
    const float s0 = state[blockIdx.x];
    const bool fresh = s0 < 0.f;   // the reset value -1: no history
    const float level = prm.level, floor_ = prm.floor;
    const double kappa = prm.kappa, alpha = prm.alpha, lambda = prm.lambda;
    const bool one_segment = n <= kAgcSegment;

    auto row_mean = [&](const float* src) {
        double acc = 0.0;
        for (int64_t i = tid; i < n; i += kAgcThreads) acc += (double)src[i];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        double tot = 0.0;
        for (int w = 0; w < kWaves; ++w) tot += red[w];
        return tot / (double)n;
    };

    Peak pcarry{fresh ? 0.f : s0, -1};
    double ccarry = (double)s0;
    if (MODE == RCFM_AGC_CARRIER && fresh && !one_segment) ccarry = row_mean(vr);

    for (int64_t g0 = 0; g0 < n; g0 += kAgcSegment) {
        const int len = (int)((n - g0 < kAgcSegment) ? (n - g0) : kAgcSegment);
        const int R = agc_run(len);
        if (VEC) {
            for (int i = 4 * tid; i < len; i += 4 * kAgcThreads)
                *reinterpret_cast<float4*>(buf + i) = *reinterpret_cast<const float4*>(vr + g0 + i);
        } else {
            for (int i = tid; i < len; i += kAgcThreads) buf[i] = vr[g0 + i];
        }
        __syncthreads();
        if (MODE == RCFM_AGC_CARRIER && fresh && one_segment) ccarry = row_mean(buf);

        const int lo = (tid * R < len) ? tid * R : len;
        const int hi = (lo + R < len) ? lo + R : len;
        if (MODE == RCFM_AGC_PEAK) {
            Peak c{0.f, (int)g0 + lo};
            double e = 0.0;   // = c.p lambda^(i - c.pos)
            for (int i = lo; i < hi; ++i) {
                const float x = fabsf(buf[i]);
                e *= lambda;
                if ((double)x >= e) {
                    e = (double)x;
                    c = Peak{x, (int)g0 + i};
                }
            }
            for (int off = 1; off < 64; off <<= 1) {   // inclusive scan of the wave's aggregates
                const Peak o{__shfl_up(c.p, off, 64), __shfl_up(c.pos, off, 64)};
                if (lane >= off) c = peak_join(o, c, kappa);
            }
            if (lane == 63) wpeak[wave] = c;
            const Peak before{__shfl_up(c.p, 1, 64), __shfl_up(c.pos, 1, 64)};
            __syncthreads();
            Peak in = pcarry;
            for (int w = 0; w < kWaves; ++w) {
                if (w == wave) in = pcarry;   // (pcarry has just taken in the waves before this one)
                pcarry = peak_join(pcarry, wpeak[w], kappa);
            }
            if (lane > 0) in = peak_join(in, before, kappa);
            e = (double)in.p * (double)agc_decay((int)g0 + lo - 1 - in.pos, kappa);   // the follower before this run
            for (int i = lo; i < hi; ++i) {
                const float x = buf[i], ax = fabsf(x);
                e *= lambda;
                if ((double)ax >= e) e = (double)ax;
                const float ef = (float)e;
                const float den = (ef > floor_) ? ef : floor_;
                buf[i] = (den > 0.f) ? clip999(level * x / den) : 0.f;
            }
        } else {
            Affine a{1.0, 0.0};
            for (int i = lo; i < hi; ++i) a.b = fma(alpha, (double)buf[i] - a.b, a.b);
            if (hi - lo == R) {
                a.d = (len == kAgcSegment) ? prm.run_full : prm.run_last;
            } else {   // the one shorter run at the segment's end (and the empty ones behind it)
                for (int i = lo; i < hi; ++i) a.d *= lambda;
            }
            for (int off = 1; off < 64; off <<= 1) {
                const Affine o{__shfl_up(a.d, off, 64), __shfl_up(a.b, off, 64)};
                if (lane >= off) a = affine_join(o, a);
            }
            if (lane == 63) waff[wave] = a;
            const Affine before{__shfl_up(a.d, 1, 64), __shfl_up(a.b, 1, 64)};
            __syncthreads();
            double c = ccarry;
            for (int w = 0; w < kWaves; ++w) {
                if (w == wave) c = ccarry;
                ccarry = fma(waff[w].d, ccarry, waff[w].b);
            }
            if (lane > 0) c = fma(before.d, c, before.b);
            for (int i = lo; i < hi; ++i) {
                const double x = (double)buf[i];
                c = fma(alpha, x - c, c);
                const double den = (c > (double)floor_) ? c : (double)floor_;
                buf[i] = (den > 0.0) ? clip999(level * (float)(x - c) / (float)den) : 0.f;
            }
        }
        __syncthreads();
        if (VEC) {
            for (int i = 4 * tid; i < len; i += 4 * kAgcThreads)
                *reinterpret_cast<float4*>(ar + g0 + i) = *reinterpret_cast<const float4*>(buf + i);
        } else {
            for (int i = tid; i < len; i += kAgcThreads) ar[g0 + i] = buf[i];
        }
        __syncthreads();   // the next segment overwrites buf and the wave totals
    }
    if (tid == 0) {
        if (MODE == RCFM_AGC_PEAK)
            state[blockIdx.x] = pcarry.p * agc_decay((int)(n - 1) - pcarry.pos, kappa);
        else
            state[blockIdx.x] = (float)ccarry;
    }
}

}  // namespace

void launch_agc_tail(int mode, const float* v, float* audio, int64_t n, int batch, const AgcParams& prm, float* state,
                     hipStream_t stream) {
    if (batch <= 0 || n <= 0) return;
    AgcArgs p;
    p.alpha = -std::expm1(-1.0 / prm.decay_samples);
    p.lambda = std::exp(-1.0 / prm.decay_samples);
    p.kappa = 1.4426950408889634 / prm.decay_samples;
    const int last = (int)(n % kAgcSegment);
    p.run_full = std::exp(-(double)agc_run(kAgcSegment) / prm.decay_samples);
    p.run_last = std::exp(-(double)agc_run(last ? last : kAgcSegment) / prm.decay_samples);
    p.level = prm.level;
    p.floor = prm.floor;
    const bool vec = n % 4 == 0 && (((uintptr_t)v | (uintptr_t)audio) & 15) == 0;
    const dim3 grid((unsigned)batch), block(kAgcThreads);
    if (mode == RCFM_AGC_PEAK) {
        if (vec)
            hipLaunchKernelGGL((k_agc_tail<RCFM_AGC_PEAK, true>), grid, block, 0, stream, v, audio, n, p, state);
        else
            hipLaunchKernelGGL((k_agc_tail<RCFM_AGC_PEAK, false>), grid, block, 0, stream, v, audio, n, p, state);
    } else {
        if (vec)
            hipLaunchKernelGGL((k_agc_tail<RCFM_AGC_CARRIER, true>), grid, block, 0, stream, v, audio, n, p, state);
        else
            hipLaunchKernelGGL((k_agc_tail<RCFM_AGC_CARRIER, false>), grid, block, 0, stream, v, audio, n, p, state);
    }
    RC_HIP(hipGetLastError());
}

}  // namespace rcfm
