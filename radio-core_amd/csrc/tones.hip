// The tone bank (rcfm_tone_bank_*, rcfm_tone_score; include/rcfm.h, "tone bank"): per channel and time frame of the audio,
// the power at each of K given frequencies and the frame's total power.  A skinny real-by-complex matrix product on the
// vector ALU: k_tone_bank for a (channel, frame, segment), k_tone_finish where a frame has several segments, k_tone_score
// for the tone squelch's ratio.
#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "tones.h"

namespace rcfm {

namespace {

constexpr int kMaxGridY = 65535;

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);     // a fixed tree: every lane ends with the same sum
    return v;
}

// Tone k's offset into the fine table, made to depend on `after`, a value of the loop iteration.  Left to itself the
// compiler hoists all 256 scalar loads of a wave's table out of the chunk loop, runs out of scalar registers and reads the
// values back lane by lane (v_readlane: 3.5 of them per FMA).  Ordered behind the sums of tone k - 2, the loads of tone
// k + 1 are in flight while tone k computes, and two tones' values are live at a time.  The results do not depend on it,
// the speed does (a factor of 2.8 on the CTCSS bank), and it is one compiler version's behaviour that it answers: after a
// toolchain update look at the listing of k_tone_bank (hipcc -S --cuda-device-only) -- its chunk loop holds 16
// s_load_dwordx16 and four v_readlane_b32; hundreds of v_readlane_b32 there are the old form back -- or run
// tools/tone_band.py, which warns when the CTCSS bank falls below 0.3 of the vector peak (0.44 measured, 0.15 hoisted).
__device__ __forceinline__ int fine_offset(int k, float& after) {
    int off = k * kToneChunk;
    asm volatile("" : "+s"(off), "+v"(after));
    return off;
}

// One workgroup: segment `seg` (kToneSegment samples, the last one shorter) of frame f of channel blockIdx.y; wave v of it
// owns tones [8 v, 8 v + 8).  The workgroup stages x w of the segment into LDS once, kToneChunk samples to a chunk, chunks
// kToneChunkPad floats apart, and adds up x^2 on the way (in float64: one FMA per sample, against 2 K for the tones).
// Lane l of every wave then takes chunks l and l + 64, l + 128 and l + 192, ... two at a time: per chunk and tone 2 x 16
// FMAs against the fine table and one complex multiply-add by the chunk's coarse phasor; the lanes' sums fold in a fixed
// tree.  The fine table's addresses are wave-uniform: it comes through the scalar cache, a tone's 32 floats at a time, and
// each value feeds the FMAs of both chunks (fine_offset below keeps those loads inside the loop).
// Sum order: a function of L alone for P, of (L, K) for E (K sets the number of staging threads).
// nseg == 1: the workgroup writes P and E itself; otherwise its sums go to part_z / part_e for k_tone_finish.
__global__ void __launch_bounds__(kToneMaxK / kToneBlock * 64)
k_tone_bank(const float* __restrict__ audio, size_t row, int step, int offset, int L, int F, int nseg, int K, int Kp,
            int ncoarse, const float* __restrict__ w, const float2* __restrict__ fine, const float2* __restrict__ coarse,
            double inv_s2, double inv_l, float* __restrict__ P, float* __restrict__ E, float2* __restrict__ part_z,
            double* __restrict__ part_e) {
    __shared__ __align__(16) float xs[kToneSegChunks * kToneChunkPad];
    __shared__ double esum[kToneMaxK / kToneBlock];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int f = blockIdx.x / nseg, seg = blockIdx.x - f * nseg;
    const int s0 = seg * kToneSegment;                                 // first sample of the segment inside its frame
    const int n = min(kToneSegment, L - s0);
    const int nch = (n + kToneChunk - 1) / kToneChunk;
    const float* src = audio + (size_t)blockIdx.y * row + ((size_t)f * L + s0) * step + offset;
    const float* wv = w + s0;                                          // 16-byte aligned: s0 is a multiple of kToneSegment
    const bool vec = step == 1 && reinterpret_cast<uintptr_t>(src) % 16 == 0;
    double e2 = 0.0;
    for (int g = tid; g < 4 * nch; g += nthreads) {                    // groups of four samples; zeros behind sample n
        const int i = 4 * g;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), ww = x;
        if (vec && i + 4 <= n) {
            x = *reinterpret_cast<const float4*>(src + i);
            ww = *reinterpret_cast<const float4*>(wv + i);
        } else {
            if (i + 0 < n) x.x = src[(size_t)(i + 0) * step], ww.x = wv[i + 0];
            if (i + 1 < n) x.y = src[(size_t)(i + 1) * step], ww.y = wv[i + 1];
            if (i + 2 < n) x.z = src[(size_t)(i + 2) * step], ww.z = wv[i + 2];
            if (i + 3 < n) x.w = src[(size_t)(i + 3) * step], ww.w = wv[i + 3];
        }
        e2 = fma((double)x.x, (double)x.x, e2);
        e2 = fma((double)x.y, (double)x.y, e2);
        e2 = fma((double)x.z, (double)x.z, e2);
        e2 = fma((double)x.w, (double)x.w, e2);
        *reinterpret_cast<float4*>(xs + (i / kToneChunk) * kToneChunkPad + (i % kToneChunk)) =
            make_float4(x.x * ww.x, x.y * ww.y, x.z * ww.z, x.w * ww.w);
    }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    e2 = wave_sum(e2);
    if (lane == 0) esum[wave] = e2;
    __syncthreads();
    const size_t cf = (size_t)blockIdx.y * F + f;
    if (tid == 0) {
        double tot = esum[0];
        for (int v = 1; v < nthreads / 64; ++v) tot += esum[v];
        if (nseg == 1) {
            if (E != nullptr) E[cf] = (float)(tot * inv_l);
        } else {
            part_e[cf * nseg + seg] = tot;
        }
    }
    const float2* fw = fine + (size_t)wave * kToneBlock * kToneChunk;
    const float2* cw = coarse + (size_t)wave * kToneBlock * ncoarse + (size_t)seg * kToneSegChunks;
    float2 acc[kToneBlock];
#pragma unroll
    for (int k = 0; k < kToneBlock; ++k) acc[k] = make_float2(0.f, 0.f);
    for (int m = lane; m < nch; m += 128) {
        const bool two = m + 64 < nch;
        const int m1 = two ? m + 64 : m;                                // without a second chunk: zeros, at an address in bounds
        const float4* p0 = reinterpret_cast<const float4*>(xs + m * kToneChunkPad);
        const float4* p1 = reinterpret_cast<const float4*>(xs + m1 * kToneChunkPad);
        const float4 a = p0[0], b = p0[1], c = p0[2], d = p0[3];
        const float4 e = p1[0], g = p1[1], h = p1[2], o = p1[3];
        float x0[kToneChunk] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
        float x1[kToneChunk] = {e.x, e.y, e.z, e.w, g.x, g.y, g.z, g.w, h.x, h.y, h.z, h.w, o.x, o.y, o.z, o.w};
#pragma unroll
        for (int j = 0; j < kToneChunk; ++j) x1[j] = two ? x1[j] : 0.f;
#pragma unroll
        for (int k = 0; k < kToneBlock; ++k) {
            const int off = fine_offset(k, k >= 2 ? acc[k - 2].y : x0[0]);
            float sr0 = 0.f, si0 = 0.f, sr1 = 0.f, si1 = 0.f;
#pragma unroll
            for (int j = 0; j < kToneChunk; ++j) {
                const float2 t = fw[off + j];
                sr0 = fmaf(x0[j], t.x, sr0);
                si0 = fmaf(x0[j], t.y, si0);
                sr1 = fmaf(x1[j], t.x, sr1);
                si1 = fmaf(x1[j], t.y, si1);
            }
            const float2 q0 = cw[(size_t)k * ncoarse + m], q1 = cw[(size_t)k * ncoarse + m1];
            acc[k].x = fmaf(sr0, q0.x, fmaf(-si0, q0.y, acc[k].x));
            acc[k].y = fmaf(sr0, q0.y, fmaf(si0, q0.x, acc[k].y));
            acc[k].x = fmaf(sr1, q1.x, fmaf(-si1, q1.y, acc[k].x));
            acc[k].y = fmaf(sr1, q1.y, fmaf(si1, q1.x, acc[k].y));
        }
    }
#pragma unroll
    for (int k = 0; k < kToneBlock; ++k) {
        acc[k].x = wave_sum(acc[k].x);
        acc[k].y = wave_sum(acc[k].y);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kToneBlock; ++k) {
            const int kk = wave * kToneBlock + k;
            if (kk >= K) break;
            if (nseg == 1)
                P[cf * K + kk] = (float)(((double)acc[k].x * acc[k].x + (double)acc[k].y * acc[k].y) * inv_s2);
            else
                part_z[(cf * nseg + seg) * Kp + kk] = acc[k];
        }
    }
}

// Frames of several segments: thread (c f, k) adds the segments' sums in segment order; k == K is the energy.
__global__ void __launch_bounds__(kToneScoreThreads)
k_tone_finish(const float2* __restrict__ part_z, const double* __restrict__ part_e, size_t frames, int nseg, int K, int Kp,
              double inv_s2, double inv_l, float* __restrict__ P, float* __restrict__ E) {
    const size_t id = (size_t)blockIdx.x * kToneScoreThreads + threadIdx.x;
    const size_t cf = id / (size_t)(K + 1);
    const int k = (int)(id - cf * (size_t)(K + 1));
    if (cf >= frames) return;
    if (k < K) {
        float2 z = part_z[cf * nseg * Kp + k];
        for (int s = 1; s < nseg; ++s) {
            const float2 t = part_z[(cf * nseg + s) * Kp + k];
            z.x += t.x;
            z.y += t.y;
        }
        P[cf * K + k] = (float)(((double)z.x * z.x + (double)z.y * z.y) * inv_s2);
    } else if (E != nullptr) {
        double tot = part_e[cf * nseg];
        for (int s = 1; s < nseg; ++s) tot += part_e[cf * nseg + s];
        E[cf] = (float)(tot * inv_l);
    }
}

// One thread per channel: the largest P / E of the wanted tone over the frames.
__global__ void __launch_bounds__(kToneScoreThreads)
k_tone_score(const float* __restrict__ P, const float* __restrict__ E, const int32_t* __restrict__ want,
             const uint8_t* __restrict__ gate, int count, int F, int K, float* __restrict__ score) {
    const int c = blockIdx.x * kToneScoreThreads + threadIdx.x;
    if (c >= count) return;
    const int k = want[c];
    float s;
    if ((gate != nullptr && gate[c] == 0) || k < -1 || k >= K) {
        s = __builtin_nanf("");
    } else if (k == -1) {
        s = __builtin_inff();
    } else {
        s = 0.f;
        for (int f = 0; f < F; ++f) {
            const float e = E[(size_t)c * F + f];
            const float r = e == 0.f ? 0.f : P[((size_t)c * F + f) * K + k] / e;
            s = fmaxf(s, r);                                            // a NaN ratio never wins
        }
    }
    score[c] = s;
}

// exp(-2 pi j frac(nu i)), frac in float64, rounded to complex64 once
float2 phasor(double nu, int64_t i) {
    const double t = nu * (double)i;
    const double a = -2.0 * M_PI * (t - std::floor(t));
    return make_float2((float)std::cos(a), (float)std::sin(a));
}

}  // namespace

}  // namespace rcfm

using namespace rcfm;

struct rcfm_tone_bank_s {
    int K = 0, Kp = 0, L = 0, nseg = 0, ncoarse = 0;
    double inv_s2 = 0.0, inv_l = 0.0;
    DeviceBuffer w, fine, coarse;          // float32 [L]; complex64 [Kp][kToneChunk]; complex64 [Kp][ncoarse]
    // partial sums of frames with several segments, one buffer per stream that has run such a bank: calls on one stream
    // are ordered, calls on different streams never share one (two lanes may run one bank)
    std::mutex mu;
    std::map<hipStream_t, DeviceBuffer> part;

    void* partials(hipStream_t s, size_t bytes) {
        std::lock_guard<std::mutex> lock(mu);
        DeviceBuffer& b = part[s];
        b.reserve(bytes);
        return b.get();
    }
};

extern "C" {

int rcfm_tone_bank_create(int K, const double* nu_host, int L, const float* window_host, rcfm_tone_bank_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr && nu_host != nullptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(K >= 1 && K <= kToneMaxK, RCFM_ERR_ARG, "a tone bank holds 1 .. 64 tones");
        RC_REQUIRE(L >= 1 && L <= kToneMaxL, RCFM_ERR_ARG, "frame length outside 1 .. 2^24");
        for (int k = 0; k < K; ++k)
            RC_REQUIRE(std::isfinite(nu_host[k]) && nu_host[k] >= 0.0 && nu_host[k] <= 0.5, RCFM_ERR_ARG,
                       "a tone frequency is not finite or outside 0 .. 0.5 cycles per sample");
        double S = (double)L;
        if (window_host != nullptr) {
            S = 0.0;
            for (int i = 0; i < L; ++i) {
                RC_REQUIRE(std::isfinite(window_host[i]), RCFM_ERR_ARG, "a window element is not finite");
                S += (double)window_host[i];
            }
            RC_REQUIRE(S > 0.0, RCFM_ERR_ARG, "the window's sum must be positive");
        }
        auto b = std::make_unique<rcfm_tone_bank_s>();
        b->K = K;
        b->Kp = tone_padded(K);
        b->L = L;
        b->nseg = tone_segments(L);
        b->ncoarse = tone_chunks(L);
        b->inv_s2 = 1.0 / (S * S);
        b->inv_l = 1.0 / (double)L;
        std::vector<float> w((size_t)L, 1.0f);
        if (window_host != nullptr) std::copy(window_host, window_host + L, w.begin());
        // tones beyond K are zeros: their sums are never written
        std::vector<float2> fine((size_t)b->Kp * kToneChunk, make_float2(0.f, 0.f));
        std::vector<float2> coarse((size_t)b->Kp * b->ncoarse, make_float2(0.f, 0.f));
        for (int k = 0; k < K; ++k) {
            for (int j = 0; j < kToneChunk; ++j) fine[(size_t)k * kToneChunk + j] = phasor(nu_host[k], j);
            for (int m = 0; m < b->ncoarse; ++m) coarse[(size_t)k * b->ncoarse + m] = phasor(nu_host[k], (int64_t)m * kToneChunk);
        }
        b->w.upload(w.data(), w.size() * sizeof(float));
        b->fine.upload(fine.data(), fine.size() * sizeof(float2));
        b->coarse.upload(coarse.data(), coarse.size() * sizeof(float2));
        *out = b.release();
    });
}

int rcfm_tone_bank_run(rcfm_tone_bank_t b, const void* audio, int count, int A, int step, int offset, void* power, void* energy,
                       void* stream) {
    return guarded([&] {
        RC_REQUIRE(b && audio && power, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(count >= 1 && A >= 1, RCFM_ERR_ARG, "count and A must be at least 1");
        RC_REQUIRE((step == 1 || step == 2) && offset >= 0 && offset < step, RCFM_ERR_ARG, "step is 1 or 2, 0 <= offset < step");
        RC_REQUIRE((uintptr_t)audio % 4 == 0 && (uintptr_t)power % 4 == 0 && (uintptr_t)energy % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: audio, power and energy are aligned for a float");
        RC_REQUIRE(A >= b->L, RCFM_ERR_SIZE, "the audio row is shorter than one frame");
        const int F = A / b->L, nseg = b->nseg;
        const size_t row = (size_t)A * (size_t)step;
        RC_REQUIRE((size_t)F * (size_t)nseg <= 0x7fffffffu, RCFM_ERR_ARG, "too many frames");
        hipStream_t s = as_stream(stream);
        const float* a = static_cast<const float*>(audio);
        float* P = static_cast<float*>(power);
        float* E = static_cast<float*>(energy);
        const dim3 block((unsigned)(tone_waves(b->K) * 64));
        const size_t per_channel = (size_t)F * nseg * ((size_t)b->Kp * sizeof(float2) + sizeof(double));
        float2* part_z = nullptr;
        double* part_e = nullptr;
        if (nseg > 1) {
            const size_t most = (size_t)std::min(count, kMaxGridY);
            part_z = static_cast<float2*>(b->partials(s, most * per_channel));
            part_e = reinterpret_cast<double*>(part_z + most * F * nseg * b->Kp);
        }
        for (int c0 = 0; c0 < count; c0 += kMaxGridY) {                 // channels are a grid coordinate
            const int cnt = std::min(kMaxGridY, count - c0);
            float* Pc = P + (size_t)c0 * F * b->K;
            float* Ec = E != nullptr ? E + (size_t)c0 * F : nullptr;
            hipLaunchKernelGGL(k_tone_bank, dim3((unsigned)(F * nseg), (unsigned)cnt), block, 0, s, a + (size_t)c0 * row, row, step,
                               offset, b->L, F, nseg, b->K, b->Kp, b->ncoarse, b->w.as<float>(), b->fine.as<float2>(),
                               b->coarse.as<float2>(), b->inv_s2, b->inv_l, Pc, Ec, part_z, part_e);
            RC_HIP(hipGetLastError());
            if (nseg > 1) {
                const size_t frames = (size_t)cnt * F, items = frames * (size_t)(b->K + 1);
                hipLaunchKernelGGL(k_tone_finish, dim3((unsigned)((items + kToneScoreThreads - 1) / kToneScoreThreads)),
                                   dim3(kToneScoreThreads), 0, s, part_z, part_e, frames, nseg, b->K, b->Kp, b->inv_s2, b->inv_l,
                                   Pc, Ec);
                RC_HIP(hipGetLastError());
            }
        }
    });
}

int rcfm_tone_bank_destroy(rcfm_tone_bank_t b) {
    return guarded([&] { delete b; });
}

int rcfm_tone_score(const void* power, const void* energy, const void* want, const void* gate, int count, int F, int K,
                    void* score, void* stream) {
    return guarded([&] {
        RC_REQUIRE(power && energy && want && score, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(count >= 1 && F >= 1, RCFM_ERR_ARG, "count and F must be at least 1");
        RC_REQUIRE(K >= 1 && K <= kToneMaxK, RCFM_ERR_ARG, "a tone bank holds 1 .. 64 tones");
        RC_REQUIRE((uintptr_t)power % 4 == 0 && (uintptr_t)energy % 4 == 0 && (uintptr_t)want % 4 == 0 && (uintptr_t)score % 4 == 0,
                   RCFM_ERR_ARG, "misaligned buffer: power, energy and score are aligned for a float, want for an int32");
        hipLaunchKernelGGL(k_tone_score, dim3((unsigned)((count + kToneScoreThreads - 1) / kToneScoreThreads)),
                           dim3(kToneScoreThreads), 0, as_stream(stream), static_cast<const float*>(power),
                           static_cast<const float*>(energy), static_cast<const int32_t*>(want), static_cast<const uint8_t*>(gate),
                           count, F, K, static_cast<float*>(score));
        RC_HIP(hipGetLastError());
    });
}

}  // extern "C"
