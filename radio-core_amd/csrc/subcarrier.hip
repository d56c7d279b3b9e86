// The subcarrier tap (rcfm_subcarrier_*, include/rcfm.h): per channel, the FM multiplex mixed down by f, low-pass filtered
// and decimated by D = B / R.  One kernel, k_subcarrier_tap<FROM_PHASE>, for channels the tuner left as phases or as
// samples; k_subcarrier_tap_single for the (D, T) whose smallest tile does not fit the LDS (subcarrier.h).
#include <cmath>
#include <cstring>

#include "api_internal.h"
#include "device_math.h"
#include "subcarrier.h"

namespace rcfm {

namespace {

// angle(x[n]) / pi of row `in`, n inside [0, B)
template <bool FROM_PHASE>
__device__ __forceinline__ float load_theta(const void* in, int64_t n) {
    if (FROM_PHASE) return static_cast<const float*>(in)[n];
    const float2 x = static_cast<const float2*>(in)[n];
    return atan2_over_pi(x.y, x.x);
}

// th[1 + e] = theta of samples nb + e, e = 0 .. 3 (zero outside the row), th[0] = theta of nb - 1 (zero for nb = 0).
// One 16-byte load (two for samples) where the group lies inside the row and `vec` says rows are 16-byte aligned.
template <bool FROM_PHASE>
__device__ __forceinline__ void load_group(const void* in, int64_t nb, int B, bool vec, float (&th)[5]) {
    th[0] = nb >= 1 && nb - 1 < B ? load_theta<FROM_PHASE>(in, nb - 1) : 0.f;
    if (vec && nb >= 0 && nb + 4 <= B) {
        if (FROM_PHASE) {
            const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(in) + nb);
            th[1] = v.x, th[2] = v.y, th[3] = v.z, th[4] = v.w;
        } else {
            const float4* p = reinterpret_cast<const float4*>(static_cast<const float2*>(in) + nb);
            const float4 a = p[0], b = p[1];
            th[1] = atan2_over_pi(a.y, a.x), th[2] = atan2_over_pi(a.w, a.z);
            th[3] = atan2_over_pi(b.y, b.x), th[4] = atan2_over_pi(b.w, b.z);
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) th[1 + e] = nb + e >= 0 && nb + e < B ? load_theta<FROM_PHASE>(in, nb + e) : 0.f;
}

// One workgroup: J consecutive outputs of one channel.  It stages the discriminator d of the samples they need -- and
// zeros for what lies before and behind the row or is not needed -- into LDS by polyphase component: sample m of the tile
// goes to row m mod D, column m div D, so output j reads tap i = p + r D at row p, column j + r, consecutive for
// consecutive outputs.  A thread owns four consecutive outputs and walks each row four taps at a time: one 16-byte LDS read
// feeds 32 FMAs.  Taps are uniform: they come through the scalar cache.  Sum order: rows ascending, taps ascending.
template <bool FROM_PHASE>
__global__ void __launch_bounds__(kTapThreads)
k_subcarrier_tap(const void* __restrict__ in_all, float2* __restrict__ out_all, const float2* __restrict__ gp,
                 const float2* __restrict__ rot, int B, int R, int D, int T, int J, int Q, int rpad, int vec_in, int vec_out) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, row = blockIdx.y;
    const int j0 = blockIdx.x * J;
    const int jt = min(J, R - j0);                                   // outputs of this tile
    const int c = (T - 1) / 2;
    const void* in = FROM_PHASE ? static_cast<const void*>(static_cast<const float*>(in_all) + (size_t)row * B)
                                : static_cast<const void*>(static_cast<const float2*>(in_all) + (size_t)row * B);
    const int64_t n0 = (int64_t)j0 * D - c;                         // sample of LDS cell (0, 0)
    const int total = D * Q;
    const int64_t lo = max(n0, (int64_t)1);                          // d[0] = 0
    const int64_t hi = min(n0 + (int64_t)(jt - 1) * D + T, (int64_t)B);
    const int64_t k0 = (n0 >= 0 ? n0 : n0 - 3) / 4;                  // floor
    const int groups = (int)((n0 + total + 3) / 4 - k0);
    // a batch of groups per thread: every load of the batch is in flight before the first LDS write waits for one
    for (int g0 = tid; g0 < groups; g0 += kTapStageBatch * kTapThreads) {
        float th[kTapStageBatch][5];
#pragma unroll
        for (int b = 0; b < kTapStageBatch; ++b) {
            const int64_t nb = 4 * (k0 + g0 + b * kTapThreads);
            if (g0 + b * kTapThreads < groups && nb + 4 > lo && nb < hi) load_group<FROM_PHASE>(in, nb, B, vec_in != 0, th[b]);
        }
#pragma unroll
        for (int b = 0; b < kTapStageBatch; ++b) {
            if (g0 + b * kTapThreads >= groups) break;
            const int64_t nb = 4 * (k0 + g0 + b * kTapThreads);
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            if (nb + 4 > lo && nb < hi) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (nb + e >= lo && nb + e < hi) d[e] = phase_step_wrapped(th[b][1 + e], th[b][e]);
            }
            int m = (int)(nb - n0);                                  // -3 .. total - 1
            int q = m >= 0 ? m / D : 0, p = m >= 0 ? m - q * D : 0;
#pragma unroll
            for (int e = 0; e < 4; ++e, ++m) {
                if (m < 0 || m >= total) continue;
                lds[p * Q + q] = d[e];
                if (++p == D) p = 0, ++q;
            }
        }
    }
    __syncthreads();
    const int jl = kTapBlock * tid;
    if (jl >= jt) return;
    float2 acc[kTapBlock];
#pragma unroll
    for (int k = 0; k < kTapBlock; ++k) acc[k] = make_float2(0.f, 0.f);
    const int rows = min(D, T);
    for (int p = 0; p < rows; ++p) {
        const float* cell = lds + p * Q + jl;
        const float2* taps = gp + (size_t)p * rpad;
        const int steps = ((T - p + D - 1) / D + kTapBlock - 1) / kTapBlock;
        float4 w = *reinterpret_cast<const float4*>(cell);
        float4 nx = *reinterpret_cast<const float4*>(cell + 4);
        for (int st = 0; st < steps; ++st) {
            const float4 ahead = *reinterpret_cast<const float4*>(cell + 4 * st + 8);
            const float v[7] = {w.x, w.y, w.z, w.w, nx.x, nx.y, nx.z};
#pragma unroll
            for (int s = 0; s < kTapBlock; ++s) {
                const float2 t = taps[4 * st + s];
#pragma unroll
                for (int k = 0; k < kTapBlock; ++k) {
                    acc[k].x = fmaf(t.x, v[k + s], acc[k].x);
                    acc[k].y = fmaf(t.y, v[k + s], acc[k].y);
                }
            }
            w = nx;
            nx = ahead;
        }
    }
    float2* out = out_all + (size_t)row * R + j0 + jl;
    float2 y[kTapBlock];
#pragma unroll
    for (int k = 0; k < kTapBlock; ++k) {
        const float2 r = jl + k < jt ? rot[j0 + jl + k] : make_float2(0.f, 0.f);
        y[k].x = fmaf(acc[k].x, r.x, -(acc[k].y * r.y));
        y[k].y = fmaf(acc[k].x, r.y, acc[k].y * r.x);
    }
    if (vec_out && jl + kTapBlock <= jt) {
        float4* o = reinterpret_cast<float4*>(out);
        o[0] = make_float4(y[0].x, y[0].y, y[1].x, y[1].y);
        o[1] = make_float4(y[2].x, y[2].y, y[3].x, y[3].y);
    } else {
#pragma unroll
        for (int k = 0; k < kTapBlock; ++k)
            if (jl + k < jt) out[k] = y[k];
    }
}

// One workgroup per output, for the (D, T) with no tile (D beyond a few thousand: outputs share few inputs or none).
// Thread t adds taps t, t + 256, ... in ascending order; the 256 partial sums fold in a fixed tree.
template <bool FROM_PHASE>
__global__ void __launch_bounds__(kTapThreads)
k_subcarrier_tap_single(const void* __restrict__ in_all, float2* __restrict__ out_all, const float2* __restrict__ g,
                        const float2* __restrict__ rot, int B, int R, int D, int T) {
    __shared__ float2 part[kTapThreads];
    const int tid = threadIdx.x, row = blockIdx.y, j = blockIdx.x;
    const int c = (T - 1) / 2;
    const void* in = FROM_PHASE ? static_cast<const void*>(static_cast<const float*>(in_all) + (size_t)row * B)
                                : static_cast<const void*>(static_cast<const float2*>(in_all) + (size_t)row * B);
    const int64_t n0 = (int64_t)j * D - c;
    float2 acc = make_float2(0.f, 0.f);
    for (int i = tid; i < T; i += kTapThreads) {
        const int64_t n = n0 + i;
        float d = 0.f;
        if (n >= 1 && n < B) d = phase_step_wrapped(load_theta<FROM_PHASE>(in, n), load_theta<FROM_PHASE>(in, n - 1));
        const float2 t = g[i];
        acc.x = fmaf(t.x, d, acc.x);
        acc.y = fmaf(t.y, d, acc.y);
    }
    part[tid] = acc;
    __syncthreads();
    for (int half = kTapThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
            part[tid].x += part[tid + half].x;
            part[tid].y += part[tid + half].y;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float2 a = part[0], r = rot[j];
        out_all[(size_t)row * R + j] = make_float2(fmaf(a.x, r.x, -(a.y * r.y)), fmaf(a.x, r.y, a.y * r.x));
    }
}

}  // namespace

void launch_subcarrier_tap(const void* in, bool from_phase, float2* out, const float2* g, const float2* gp, const float2* rot,
                           int B, int R, int T, int count, hipStream_t s) {
    if (count <= 0) return;
    const int D = B / R;
    const TapTile tile = tap_tile(D, T);
    if (tile.J == 0) {
        const dim3 grid((unsigned)R, (unsigned)count);
        if (from_phase)
            hipLaunchKernelGGL(k_subcarrier_tap_single<true>, grid, dim3(kTapThreads), 0, s, in, out, g, rot, B, R, D, T);
        else
            hipLaunchKernelGGL(k_subcarrier_tap_single<false>, grid, dim3(kTapThreads), 0, s, in, out, g, rot, B, R, D, T);
        RC_HIP(hipGetLastError());
        return;
    }
    // 16-byte accesses where every row starts on a 16-byte boundary
    const size_t in_row = (size_t)B * (from_phase ? sizeof(float) : sizeof(float2));
    const int vec_in = reinterpret_cast<uintptr_t>(in) % 16 == 0 && in_row % 16 == 0;
    const int vec_out = reinterpret_cast<uintptr_t>(out) % 16 == 0 && ((size_t)R * sizeof(float2)) % 16 == 0;
    const dim3 grid((unsigned)((R + tile.J - 1) / tile.J), (unsigned)count);
    const dim3 block(kTapThreads);
    const size_t lds = tile.lds_bytes(D);
    if (from_phase)
        hipLaunchKernelGGL(k_subcarrier_tap<true>, grid, block, lds, s, in, out, gp, rot, B, R, D, T, tile.J, tile.Q, tile.rpad,
                           vec_in, vec_out);
    else
        hipLaunchKernelGGL(k_subcarrier_tap<false>, grid, block, lds, s, in, out, gp, rot, B, R, D, T, tile.J, tile.Q, tile.rpad,
                           vec_in, vec_out);
    RC_HIP(hipGetLastError());
}

}  // namespace rcfm

using namespace rcfm;

// ---- the handle ------------------------------------------------------------------------------------------------------------

struct rcfm_subcarrier_s {
    int C = 0, B = 0, R = 0, T = 0, chunk = 1;
    int64_t f = 0;
    DeviceBuffer g, gp, rot;     // complex64 [T], [min(D, T)][rpad], [R]
    DeviceBuffer work;           // rcfm_pipeline_subcarrier: float32 (phases) or complex64 (samples) [chunk][B]; plain device memory

    void run(int count, const void* in, bool from_phase, float2* out, hipStream_t s) const {
        launch_subcarrier_tap(in, from_phase, out, g.as<float2>(), gp.as<float2>(), rot.as<float2>(), B, R, T, count, s);
    }
};

namespace {

// exp(-2 pi i (k f mod B) / B), the product reduced exactly in 64-bit integers (|k| < 2^31, |f| <= 2^30)
// in float64: the caller rounds to float32 once
void mixer(int64_t k, int64_t f, int64_t B, double* re, double* im) {
    int64_t r = (k * f) % B;
    if (r < 0) r += B;
    const double a = -2.0 * kPi * (double)r / (double)B;
    *re = std::cos(a);
    *im = std::sin(a);
}

}  // namespace

extern "C" {

int rcfm_subcarrier_create(int C, int B, int R, int64_t f, const float* taps_host, int ntaps, int chunk, rcfm_subcarrier_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr && taps_host != nullptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1 && B >= 2 && R >= 1, RCFM_ERR_ARG, "bad subcarrier tap size");
        RC_REQUIRE(B % R == 0, RCFM_ERR_ARG, "the output length must divide the input length");
        RC_REQUIRE(f >= -(int64_t)(B / 2) && f <= (int64_t)(B / 2), RCFM_ERR_ARG, "subcarrier frequency beyond half the sample rate");
        RC_REQUIRE(ntaps >= 1 && ntaps <= 4095 && ntaps % 2 == 1, RCFM_ERR_ARG, "the number of taps must be odd, 1 .. 4095");
        for (int i = 0; i < ntaps; ++i) RC_REQUIRE(std::isfinite(taps_host[i]), RCFM_ERR_ARG, "a tap is not finite");
        auto h = std::make_unique<rcfm_subcarrier_s>();
        h->C = C;
        h->B = B;
        h->R = R;
        h->T = ntaps;
        h->f = f;
        if (chunk <= 0) chunk = (int)std::min<int64_t>(8192, std::max<int64_t>(1024, (int64_t)1024 * 240000 / B));   // rcfm_demod_create's rule
        h->chunk = std::min(std::min(chunk, C), 65535);   // channels are a grid coordinate
        const int D = B / R, T = ntaps, c = (T - 1) / 2;
        std::vector<float2> g((size_t)T), rot((size_t)R);
        for (int i = 0; i < T; ++i) {
            double re, im;
            mixer(i - c, f, B, &re, &im);
            const double hr = (double)taps_host[i];
            g[i] = make_float2((float)(hr * re), (float)(hr * im));
        }
        for (int j = 0; j < R; ++j) {
            double re, im;
            mixer((int64_t)j * D, f, B, &re, &im);
            rot[j] = make_float2((float)re, (float)im);
        }
        const TapTile tile = tap_tile(D, T);
        const int rows = std::min(D, T);
        std::vector<float2> gp((size_t)rows * tile.rpad, make_float2(0.f, 0.f));
        for (int i = 0; i < T; ++i) gp[(size_t)(i % D) * tile.rpad + i / D] = g[i];
        h->g.upload(g.data(), g.size() * sizeof(float2));
        h->gp.upload(gp.data(), gp.size() * sizeof(float2));
        h->rot.upload(rot.data(), rot.size() * sizeof(float2));
        *out = h.release();
    });
}

int rcfm_subcarrier_run(rcfm_subcarrier_t h, int count, const void* iq, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h && iq && out, RCFM_ERR_ARG, "NULL argument");
        require_channels(0, count, h->C);
        const float2* in = static_cast<const float2*>(iq);
        float2* y = static_cast<float2*>(out);
        for (int off = 0; off < count; off += h->chunk) {
            const int cnt = std::min(h->chunk, count - off);
            h->run(cnt, in + (size_t)off * h->B, false, y + (size_t)off * h->R, as_stream(stream));
        }
    });
}

int rcfm_pipeline_subcarrier(rcfm_tuner_t t, rcfm_subcarrier_t h, int first, int count, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(t && h && out, RCFM_ERR_ARG, "NULL argument");
        require_channels(first, count, t->nch);
        RC_REQUIRE(count <= h->C, RCFM_ERR_INDEX, "more channels than the subcarrier handle was created for");
        for (int i = 0; i < count; ++i)
            RC_REQUIRE(t->bw[first + i] == h->B, RCFM_ERR_SIZE, "input_sig size and input_size mismatch");
        t->require_loaded(first, count, "rcfm_pipeline_subcarrier");
        if (count == 0) return;
        hipStream_t s = as_stream(stream);
        const bool phases = t->phase_capable(first);
        // no ArenaScope is open here: the workspace is plain device memory whatever arena the tuner lives in
        h->work.reserve((size_t)h->chunk * h->B * (phases ? sizeof(float) : sizeof(float2)));
        float2* y = static_cast<float2*>(out);
        for (int off = 0; off < count; off += h->chunk) {
            const int c0 = first + off, cnt = std::min(h->chunk, count - off);
            {
                ArenaScope ts(t->arena);
                if (phases) t->run(c0, cnt, nullptr, s, h->work.as<float>(), 0);
                else t->run(c0, cnt, h->work.as<float2>(), s);
            }
            h->run(cnt, h->work.get(), phases, y + (size_t)off * h->R, s);
        }
    });
}

int rcfm_subcarrier_describe(int D, int T, int* J, int* rpad, int* Q, int64_t* lds_bytes) {
    return guarded([&] {
        RC_REQUIRE(J && rpad && Q && lds_bytes, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(D >= 1, RCFM_ERR_ARG, "bad subcarrier tap size");
        RC_REQUIRE(T >= 1 && T <= 4095 && T % 2 == 1, RCFM_ERR_ARG, "the number of taps must be odd, 1 .. 4095");
        const TapTile tile = tap_tile(D, T);
        *J = tile.J;
        *rpad = tile.rpad;
        *Q = tile.Q;
        *lds_bytes = (int64_t)tile.lds_bytes(D);
    });
}

int rcfm_subcarrier_destroy(rcfm_subcarrier_t h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
