// The per-channel audio filter (include/rcfm.h, rcfm_audio_filter_*): S biquad sections in transposed direct form II along
// every row of the audio, all of it in float64, the state (z0, z1) per channel, leg and section carried from call to call.
// The mapping is the AGC tail's (agc.hip): runs, aggregates, an ordered scan, a second sweep -- with a 2-vector of state
// where the AGC has a scalar.

#include "audio_filter.h"

#include <cmath>
#include <memory>
#include <vector>

#include "common.h"

namespace rcfm {

namespace {

struct V2 {
    double x, y;
};

// P v + add, P row-major 2 x 2
__device__ __forceinline__ V2 affine(const double* __restrict__ P, V2 v, V2 add) {
    return V2{fma(P[0], v.x, fma(P[1], v.y, add.x)), fma(P[2], v.x, fma(P[3], v.y, add.y))};
}

// One step of a section: y = b0 u + z0, then the two state updates.  Returns y.  The feed-forward terms b1 u + z1 and
// b2 u do not wait for y: the chain from one sample's z0 to the next one's is two FMAs long.
__device__ __forceinline__ double biquad(const SosSection& c, double u, V2& z) {
    const double y = fma(c.b0, u, z.x);
    const double f0 = fma(c.b1, u, z.y), f1 = c.b2 * u;
    z.x = fma(-c.a1, y, f0);
    z.y = fma(-c.a2, y, f1);
    return y;
}

// Row blockIdx.x of in [count][n][CH] -> out, with the state of channel blockIdx.x of `state` [.][CH][S][2].
// The row passes through LDS in segments of kSosSegment floats (kSosSegment / CH frames), each float read from memory
// once and written once whatever S is.  With CH = 2 the legs lie in LDS as two planes and threads [0, 128) own the left
// leg, [128, 256) the right one.  Thread r of a leg owns frames [r R, (r + 1) R) of the segment, R = kSosRun, in
// registers as float64; a short last segment has fewer active threads.  Per section:
//   sweep 1  the recurrence over the run from zero state: its end state v_r;
//   scan     the state entering run r is s_r = M^R s_(r-1) + v_(r-1): Hillis-Steele over the wave's 64 runs with the
//            tables M^(R 2^k), the leg's waves before this one in order with M^(64 R) from the segment's carry, and
//            M^(R lane) applied to that as the product of the tables of lane's bits;
//   sweep 2  the run again from s_r, the section's output over its input (registers).  The end state of the last
//            non-empty run is the next segment's carry and, after the last segment, the stored state.
// Every run before a non-empty one is whole, so no table for a partial run is needed: what the scan gives behind the
// segment's last sample is never used.  After the last section the float64 outputs are rounded once to float32.
// VEC (n CH a multiple of 4, both blocks 16-byte aligned): 16-byte loads and stores, else 4-byte ones.
// select[row] == 0: the row is copied (out != in) or left alone, and its state is not touched.
template <int CH, bool VEC>
__global__ __launch_bounds__(kSosThreads) void k_audio_filter(const float* in, float* out, int n, int S,
                                                              const SosSection* __restrict__ sections, double* state,
                                                              const uint8_t* __restrict__ select) {
    constexpr int T = kSosThreads / CH;          // threads of a leg
    constexpr int WPL = T / 64;                  // waves of a leg
    constexpr int SEGF = kSosSegment / CH;       // frames of a segment
    constexpr int PLANE = SEGF + (CH == 2 ? kSosPlanePad : 0);
    constexpr int R = kSosRun;
    static_assert(T * R >= SEGF, "the runs of a leg's threads cover a segment");
    __shared__ __attribute__((aligned(16))) float buf[CH * PLANE];
    __shared__ V2 wtot[2][kSosThreads / 64];
    __shared__ V2 carry[CH][kSosMaxSections];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int leg = tid / T, r = tid % T, wl = wave % WPL;
    const int64_t row = (int64_t)n * CH;
    const float* src = in + (int64_t)blockIdx.x * row;
    float* dst = out + (int64_t)blockIdx.x * row;
    if (select != nullptr && select[blockIdx.x] == 0) {
        if (src != dst) {
            if (VEC) {
                for (int64_t i = 4 * (int64_t)tid; i < row; i += 4 * kSosThreads)
                    *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
            } else {
                for (int64_t i = tid; i < row; i += kSosThreads) dst[i] = src[i];
            }
        }
        return;
    }
    double* st = state + (int64_t)blockIdx.x * CH * S * 2;
    if (tid < CH * S) carry[tid / S][tid % S] = V2{st[2 * tid], st[2 * tid + 1]};
    // (the first segment's barrier orders these writes before every read)

    for (int g0 = 0; g0 < n; g0 += SEGF) {
        const int len = (n - g0 < SEGF) ? (n - g0) : SEGF;      // frames
        const int nf = len * CH;                                // floats
        const float* seg_in = src + (int64_t)g0 * CH;
        float* seg_out = dst + (int64_t)g0 * CH;
        if (VEC) {
            for (int i = 4 * tid; i < nf; i += 4 * kSosThreads) {
                const float4 x = *reinterpret_cast<const float4*>(seg_in + i);
                if (CH == 1) {
                    *reinterpret_cast<float4*>(buf + i) = x;
                } else {
                    *reinterpret_cast<float2*>(buf + i / 2) = make_float2(x.x, x.z);
                    *reinterpret_cast<float2*>(buf + PLANE + i / 2) = make_float2(x.y, x.w);
                }
            }
        } else {
            for (int i = tid; i < nf; i += kSosThreads) buf[CH == 1 ? i : (i & 1) * PLANE + (i >> 1)] = seg_in[i];
        }
        __syncthreads();

        const int lo = (r * R < len) ? r * R : len;
        const int cnt = (len - lo < R) ? (len - lo) : R;
        const bool last = cnt > 0 && lo + cnt == len;
        float* mine = buf + leg * PLANE + lo;
        double u[R];
#pragma unroll
        for (int i = 0; i < R; ++i) u[i] = (i < cnt) ? (double)mine[i] : 0.0;

        for (int s = 0; s < S; ++s) {
            const SosSection& c = sections[s];
            const V2 seg_carry = carry[leg][s];      // read before this section's barrier, rewritten behind it
            V2 z{0.0, 0.0};
            if (cnt == R) {                          // a whole run: nothing to predicate (all but the segment's last wave)
#pragma unroll
                for (int i = 0; i < R; ++i) (void)biquad(c, u[i], z);
            } else {
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (i < cnt) (void)biquad(c, u[i], z);
            }
            // inclusive scan over the wave: z = the state behind run `lane` had the wave's first run started from zero
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const V2 o{__shfl_up(z.x, 1 << k, 64), __shfl_up(z.y, 1 << k, 64)};
                if (lane >= (1 << k)) z = affine(c.P[k], o, z);
            }
            if (lane == 63) wtot[s & 1][wave] = z;
            V2 before{__shfl_up(z.x, 1, 64), __shfl_up(z.y, 1, 64)};
            if (lane == 0) before = V2{0.0, 0.0};
            __syncthreads();
            V2 e = seg_carry;                        // the state entering this wave's first run
            for (int w = 0; w < WPL; ++w)
                if (w < wl) e = affine(c.P[6], e, wtot[s & 1][leg * WPL + w]);
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if ((lane >> k) & 1) e = affine(c.P[k], e, V2{0.0, 0.0});
            z = V2{e.x + before.x, e.y + before.y};
            if (cnt == R) {
#pragma unroll
                for (int i = 0; i < R; ++i) u[i] = biquad(c, u[i], z);
            } else {
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (i < cnt) u[i] = biquad(c, u[i], z);
            }
            if (last) carry[leg][s] = z;
        }
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (i < cnt) mine[i] = (float)u[i];
        __syncthreads();
        if (VEC) {
            for (int i = 4 * tid; i < nf; i += 4 * kSosThreads) {
                float4 y;
                if (CH == 1) {
                    y = *reinterpret_cast<const float4*>(buf + i);
                } else {
                    const float2 a = *reinterpret_cast<const float2*>(buf + i / 2);
                    const float2 b = *reinterpret_cast<const float2*>(buf + PLANE + i / 2);
                    y = make_float4(a.x, b.x, a.y, b.y);
                }
                *reinterpret_cast<float4*>(seg_out + i) = y;
            }
        } else {
            for (int i = tid; i < nf; i += kSosThreads) seg_out[i] = buf[CH == 1 ? i : (i & 1) * PLANE + (i >> 1)];
        }
        __syncthreads();   // the next segment overwrites buf; the carries are complete
    }
    if (tid < CH * S) {
        const V2 z = carry[tid / S][tid % S];
        st[2 * tid] = z.x;
        st[2 * tid + 1] = z.y;
    }
}

// A (long double, row-major 2 x 2) times B
void mat_mul(const long double* A, const long double* B, long double* out) {
    const long double r[4] = {A[0] * B[0] + A[1] * B[2], A[0] * B[1] + A[1] * B[3], A[2] * B[0] + A[3] * B[2],
                              A[2] * B[1] + A[3] * B[3]};
    for (int i = 0; i < 4; ++i) out[i] = r[i];
}

}  // namespace

}  // namespace rcfm

using namespace rcfm;

struct rcfm_audio_filter_s {
    int C = 0, ch = 0, S = 0;
    DeviceBuffer sections, state;      // SosSection [S]; float64 [C][ch][S][2]
    StreamFence fence;                 // rcfm_audio_filter_set_fence
    size_t state_bytes() const { return (size_t)C * ch * S * 2 * sizeof(double); }
};

extern "C" {

int rcfm_audio_filter_create(int C, int ch, int S, const double* sos_host, rcfm_audio_filter_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr && sos_host != nullptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1, RCFM_ERR_ARG, "C must be at least 1");
        RC_REQUIRE(ch == 1 || ch == 2, RCFM_ERR_ARG, "ch is 1 or 2");
        RC_REQUIRE(S >= 1 && S <= kSosMaxSections, RCFM_ERR_ARG, "an audio filter holds 1 .. 8 sections");
        for (int i = 0; i < 6 * S; ++i)
            RC_REQUIRE(std::isfinite(sos_host[i]), RCFM_ERR_ARG, "a section's coefficient is not finite");
        for (int s = 0; s < S; ++s) {
            const double a0 = sos_host[6 * s + 3], a1 = sos_host[6 * s + 4], a2 = sos_host[6 * s + 5];
            RC_REQUIRE(a0 == 1.0, RCFM_ERR_ARG, "a section's a0 is not 1");
            RC_REQUIRE(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2, RCFM_ERR_ARG,
                       "a section is not strictly stable: |a2| < 1 and |a1| < 1 + a2");
        }
        std::vector<SosSection> sec((size_t)S);
        for (int s = 0; s < S; ++s) {
            const double* q = sos_host + 6 * s;
            SosSection& c = sec[(size_t)s];
            c = SosSection{};
            c.b0 = q[0], c.b1 = q[1], c.b2 = q[2], c.a1 = q[4], c.a2 = q[5];
            const long double M[4] = {-(long double)q[4], 1.0L, -(long double)q[5], 0.0L};
            long double P[4] = {1.0L, 0.0L, 0.0L, 1.0L};
            for (int i = 0; i < kSosRun; ++i) mat_mul(P, M, P);
            for (int k = 0; k < kSosTables; ++k) {       // M^(R 2^k); k = 6 is M^(64 R)
                for (int i = 0; i < 4; ++i) c.P[k][i] = (double)P[i];
                mat_mul(P, P, P);
            }
        }
        auto f = std::make_unique<rcfm_audio_filter_s>();
        f->C = C, f->ch = ch, f->S = S;
        f->sections.upload(sec.data(), sec.size() * sizeof(SosSection));
        f->state.reset(f->state_bytes());
        RC_HIP(hipMemset(f->state.get(), 0, f->state_bytes()));
        *out = f.release();
    });
}

int rcfm_audio_filter_run(rcfm_audio_filter_t f, int first, int count, int n, const void* in, void* out, const void* select,
                          void* stream) {
    return guarded([&] {
        RC_REQUIRE(f && in && out, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(count >= 1 && n >= 1, RCFM_ERR_ARG, "count and n must be at least 1");
        RC_REQUIRE((uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: in and out are aligned for a float");
        RC_REQUIRE(first >= 0 && (int64_t)first + count <= f->C, RCFM_ERR_INDEX, "first .. first + count is outside the filter's channels");
        hipStream_t s = as_stream(stream);
        const float* x = static_cast<const float*>(in);
        float* y = static_cast<float*>(out);
        const uint8_t* sel = static_cast<const uint8_t*>(select);
        double* st = f->state.as<double>() + (size_t)first * f->ch * f->S * 2;
        const SosSection* sec = f->sections.as<SosSection>();
        const bool vec = ((int64_t)n * f->ch) % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
        StreamFence::Scope fenced(f->fence, s);
        const dim3 grid((unsigned)count), block(kSosThreads);
        if (f->ch == 1) {
            if (vec)
                hipLaunchKernelGGL((k_audio_filter<1, true>), grid, block, 0, s, x, y, n, f->S, sec, st, sel);
            else
                hipLaunchKernelGGL((k_audio_filter<1, false>), grid, block, 0, s, x, y, n, f->S, sec, st, sel);
        } else {
            if (vec)
                hipLaunchKernelGGL((k_audio_filter<2, true>), grid, block, 0, s, x, y, n, f->S, sec, st, sel);
            else
                hipLaunchKernelGGL((k_audio_filter<2, false>), grid, block, 0, s, x, y, n, f->S, sec, st, sel);
        }
        RC_HIP(hipGetLastError());
    });
}

int rcfm_audio_filter_reset(rcfm_audio_filter_t f, void* stream) {
    return guarded([&] {
        RC_REQUIRE(f, RCFM_ERR_ARG, "NULL handle");
        RC_HIP(hipMemsetAsync(f->state.get(), 0, f->state_bytes(), as_stream(stream)));
    });
}

int rcfm_audio_filter_get_state(rcfm_audio_filter_t f, double* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(f && state_host, RCFM_ERR_ARG, "NULL argument");
        state_to_host(state_host, f->state.get(), f->state_bytes(), as_stream(stream));
    });
}

int rcfm_audio_filter_set_state(rcfm_audio_filter_t f, const double* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(f && state_host, RCFM_ERR_ARG, "NULL argument");
        state_to_device(f->state.get(), state_host, f->state_bytes(), as_stream(stream));
    });
}

int rcfm_audio_filter_set_fence(rcfm_audio_filter_t f, int on) {
    return guarded([&] {
        RC_REQUIRE(f, RCFM_ERR_ARG, "NULL handle");
        f->fence.arm(on != 0);
    });
}

int rcfm_audio_filter_destroy(rcfm_audio_filter_t f) {
    return guarded([&] { delete f; });
}

}  // extern "C"
