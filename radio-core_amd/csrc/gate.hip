// The frame gate (include/rcfm.h, "frame gate"): rcfm_frame_power, the mean power of every frame of every row -- a streaming
// read; rcfm_tuner_frame_levels, the same of the samples rcfm_tuner_run returns; rcfm_gate_run, the squelch's state machine
// over a channel's frames (hysteresis, hang time, look-ahead); rcfm_gate_apply, which zeroes the closed frames of the audio
// and ramps the edges.  No existing kernel is touched: with no gate set none of this is launched.
#include "gate.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "api_internal.h"

namespace rcfm {

namespace {

constexpr int kGateWaves = kGateThreads / 64;
constexpr int kMaxGridY = 65535;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);     // a fixed tree: every lane ends with the same sum
    return v;
}

// Four floats at p, W of them per load: p is aligned for W floats.
template <int W>
__device__ __forceinline__ float4 load4(const float* __restrict__ p) {
    if (W == 4) return *reinterpret_cast<const float4*>(p);
    if (W == 2) {
        const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
        return make_float4(a.x, a.y, b.x, b.y);
    }
    return make_float4(p[0], p[1], p[2], p[3]);
}

// Sum of squares of the floats [0, m) at p, in float64: they are taken in groups of four, group g by worker g % stride
// (this one is worker idx), element e of every group into accumulator e.  Which worker adds what, and in which order,
// depends on (m, stride) alone -- not on W, which only says how a group is fetched.
template <int W>
__device__ __forceinline__ double sum_squares(const float* __restrict__ p, int m, int idx, int stride) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int full = m >> 2;
#pragma unroll 4
    for (int g = idx; g < full; g += stride) {
        const float4 v = load4<W>(p + 4 * (size_t)g);
        a0 = fma((double)v.x, (double)v.x, a0);
        a1 = fma((double)v.y, (double)v.y, a1);
        a2 = fma((double)v.z, (double)v.z, a2);
        a3 = fma((double)v.w, (double)v.w, a3);
    }
    const int rest = m & 3;
    if (rest != 0 && full % stride == idx) {                        // the short last group, element by element
        const float* q = p + 4 * (size_t)full;
        a0 = fma((double)q[0], (double)q[0], a0);
        if (rest > 1) a1 = fma((double)q[1], (double)q[1], a1);
        if (rest > 2) a2 = fma((double)q[2], (double)q[2], a2);
    }
    return (a0 + a1) + (a2 + a3);
}

// ... with the widest load the address allows: 16 bytes per lane, else 8, else 4 (uniform over the callers of one frame).
__device__ __forceinline__ double sum_squares_any(const float* __restrict__ p, int m, int idx, int stride) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if ((a & 15) == 0) return sum_squares<4>(p, m, idx, stride);
    if ((a & 7) == 0) return sum_squares<2>(p, m, idx, stride);
    return sum_squares<1>(p, m, idx, stride);
}

// Short frames (m <= kGateWaveFloats floats): wave w of workgroup b owns frame 4 b + w, all of it.  `row`: floats of a row
// of x; frame fr = r F + f starts at float r row + f m.
__global__ __launch_bounds__(kGateThreads) void k_frame_power_wave(const float* __restrict__ x, int64_t row, int m, int F,
                                                                   int64_t frames, double L, float* __restrict__ power) {
    const int lane = threadIdx.x & 63;
    const int64_t fr = (int64_t)blockIdx.x * kGateWaves + (threadIdx.x >> 6);
    if (fr >= frames) return;                                       // (a whole wave)
    const int64_t r = fr / F, f = fr - r * F;
    const double s = wave_sum(sum_squares_any(x + r * row + f * m, m, lane, 64));
    if (lane == 0) power[fr] = (float)(s / L);
}

// Long frames: workgroup b owns segment b % nseg (kGateSegFloats floats, the last one shorter) of frame b / nseg.  Its sum
// is the waves' sums in wave order; with one segment per frame it is the frame's, else it goes to part[b].
__global__ __launch_bounds__(kGateThreads) void k_frame_power_block(const float* __restrict__ x, int64_t row, int m, int F,
                                                                    int nseg, double L, float* __restrict__ power,
                                                                    double* __restrict__ part) {
    __shared__ double red[kGateWaves];
    const int tid = threadIdx.x;
    const int64_t id = blockIdx.x, fr = id / nseg;
    const int seg = (int)(id - fr * nseg);
    const int64_t r = fr / F, f = fr - r * F;
    const int s0 = seg * kGateSegFloats;
    const int len = min(kGateSegFloats, m - s0);
    const double s = wave_sum(sum_squares_any(x + r * row + f * m + s0, len, tid, kGateThreads));
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid != 0) return;
    double tot = red[0];
    for (int w = 1; w < kGateWaves; ++w) tot += red[w];
    if (nseg == 1)
        power[fr] = (float)(tot / L);
    else
        part[id] = tot;
}

// Frames of several segments: one thread per frame adds the segments' sums in segment order.
__global__ __launch_bounds__(kGateThreads) void k_frame_power_finish(const double* __restrict__ part, int64_t frames, int nseg,
                                                                     double L, float* __restrict__ power) {
    const int64_t fr = (int64_t)blockIdx.x * kGateThreads + threadIdx.x;
    if (fr >= frames) return;
    double tot = part[fr * nseg];
    for (int s = 1; s < nseg; ++s) tot += part[fr * nseg + s];
    power[fr] = (float)(tot / L);
}

// The partial sums of frames with several segments, library-owned: one buffer per stream that has ever needed one, grown
// on demand and kept.  Calls on one stream are ordered; calls on different streams never share a buffer.
double* partials(hipStream_t stream, size_t bytes) {
    static std::mutex mu;
    static std::map<hipStream_t, DeviceBuffer> bufs;
    std::lock_guard<std::mutex> lock(mu);
    DeviceBuffer& b = bufs[stream];
    b.reserve(bytes);
    return b.as<double>();
}

// rcfm_frame_power behind its argument checks.
void frame_power(const float* x, int rows, int64_t n, int is_complex, int L, float* power, hipStream_t s) {
    const int comp = is_complex ? 2 : 1;
    const int64_t F = n / L, frames = (int64_t)rows * F;
    if (frames == 0) return;
    const int m = L * comp;
    const int nseg = gate_segments(m);
    RC_REQUIRE(F <= 0x7fffffff && frames * nseg <= 0x7fffffff, RCFM_ERR_ARG, "too many frames");
    const int64_t row = n * comp;
    if (m <= kGateWaveFloats) {
        hipLaunchKernelGGL(k_frame_power_wave, dim3((unsigned)((frames + kGateWaves - 1) / kGateWaves)), dim3(kGateThreads), 0, s,
                           x, row, m, (int)F, frames, (double)L, power);
        RC_HIP(hipGetLastError());
        return;
    }
    double* part = nseg > 1 ? partials(s, sizeof(double) * (size_t)frames * nseg) : nullptr;
    hipLaunchKernelGGL(k_frame_power_block, dim3((unsigned)(frames * nseg)), dim3(kGateThreads), 0, s, x, row, m, (int)F, nseg,
                       (double)L, power, part);
    RC_HIP(hipGetLastError());
    if (nseg > 1) {
        hipLaunchKernelGGL(k_frame_power_finish, dim3((unsigned)((frames + kGateThreads - 1) / kGateThreads)), dim3(kGateThreads),
                           0, s, part, frames, nseg, (double)L, power);
        RC_HIP(hipGetLastError());
    }
}

// One thread per channel (include/rcfm.h, rcfm_gate_run): the state machine over the frames, in order, into the mask's
// columns 1 .. F; then the look-ahead, backwards over the same columns with the distance to the next open frame.
__global__ __launch_bounds__(kGateThreads) void k_gate_run(int32_t* __restrict__ state, const float* __restrict__ power,
                                                           const float* __restrict__ open_thr,
                                                           const float* __restrict__ close_thr, int count, int F, int hang,
                                                           int lead, uint8_t* __restrict__ mask, uint8_t* __restrict__ open_any) {
    const int c = blockIdx.x * kGateThreads + threadIdx.x;
    if (c >= count) return;
    int open = state[2 * c] != 0, left = state[2 * c + 1];
    const float to = open_thr[c], tc = close_thr[c];
    const float* p = power + (size_t)c * F;
    uint8_t* row = mask + (size_t)c * (F + 1);
    row[0] = (uint8_t)open;
    int any = open;
    for (int f = 0; f < F; ++f) {
        const float v = p[f];
        if (v >= to) {
            open = 1;
            left = hang;
        } else if (open && v >= tc) {
            left = hang;
        } else if (open) {
            if (left > 0)
                --left;
            else
                open = 0;
        }
        row[f + 1] = (uint8_t)open;
    }
    state[2 * c] = open;
    state[2 * c + 1] = left;
    int d = lead + 1;                                               // frames to the next open one, lead + 1: out of reach
    for (int f = F - 1; f >= 0; --f) {
        d = row[f + 1] ? 0 : min(d + 1, lead + 1);
        const int g = d <= lead;
        row[f + 1] = (uint8_t)g;
        any |= g;
    }
    if (open_any != nullptr) open_any[c] = (uint8_t)any;
}

// What becomes of sample `pos` of a frame with gate g behind gate gp (not both 1), value x: see rcfm_gate_apply.
__device__ __forceinline__ float ramp_gain(const float* __restrict__ ramp, int R, int g, int pos) {
    return g ? ramp[pos] : ramp[R - 1 - pos];
}

// Channel blockIdx.y, audio row of `row` = A ch floats, frames of La samples.  VEC (La ch a multiple of 4, 16-byte aligned
// rows): a thread owns four floats, which lie in one frame and start on leg 0; else one float.  Open frames behind open
// frames are neither read nor written.
template <bool VEC>
__global__ __launch_bounds__(kGateThreads) void k_gate_apply(float* __restrict__ audio, const uint8_t* __restrict__ mask, int F,
                                                             int La, int ch, int64_t row, const float* __restrict__ ramp, int R) {
    const int64_t j = ((int64_t)blockIdx.x * kGateThreads + threadIdx.x) * (VEC ? 4 : 1);
    if (j >= row) return;
    const int64_t i = j / ch;                                       // the sample of the first float
    const int f = (int)(i / La), pos = (int)(i - (int64_t)f * La);
    const uint8_t* m = mask + (size_t)blockIdx.y * (F + 1);
    const int g = m[f + 1] != 0, gp = m[f] != 0;
    if (g && gp) return;
    float* a = audio + (size_t)blockIdx.y * row + j;
    if (VEC) {
        float4* a4 = reinterpret_cast<float4*>(a);
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g == gp || pos >= R) {                                  // closed, or behind the ramp
            if (!g) *a4 = zero;
            return;
        }
        const int step = ch == 2 ? 1 : 0;                           // element e is sample pos + (e >> step)
        if (pos + (3 >> step) < R) {                                // inside the ramp
            float4 v = *a4;
            v.x *= ramp_gain(ramp, R, g, pos);
            v.y *= ramp_gain(ramp, R, g, pos + (1 >> step));
            v.z *= ramp_gain(ramp, R, g, pos + (2 >> step));
            v.w *= ramp_gain(ramp, R, g, pos + (3 >> step));
            *a4 = v;
            return;
        }
        for (int e = 0; e < 4; ++e) {                               // the ramp ends inside these four
            const int q = pos + (e >> step);
            if (q < R)
                a[e] *= ramp_gain(ramp, R, g, q);
            else if (!g)
                a[e] = 0.f;
        }
    } else {
        if (g != gp && pos < R)
            *a *= ramp_gain(ramp, R, g, pos);
        else if (!g)
            *a = 0.f;
    }
}

}  // namespace

}  // namespace rcfm

using namespace rcfm;

struct rcfm_gate_s {
    int C = 0, hang = 0, lead = 0, R = 0;
    DeviceBuffer state, ramp;          // int32 [C][2]: open, hang_left; float32 [R]
    StreamFence fence;                 // rcfm_gate_set_fence
    size_t state_bytes() const { return (size_t)C * 2 * sizeof(int32_t); }
};

extern "C" {

int rcfm_frame_power(const void* x, int rows, int64_t n, int is_complex, int L, void* power, void* stream) {
    return guarded([&] {
        RC_REQUIRE(x && power, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(rows >= 0, RCFM_ERR_ARG, "negative row count");
        RC_REQUIRE(L >= 1 && (int64_t)L <= n, RCFM_ERR_ARG, "the frame length is outside 1 .. n");
        RC_REQUIRE(L <= (1 << 30), RCFM_ERR_ARG, "the frame length is above 2^30");
        RC_REQUIRE((uintptr_t)x % (is_complex ? 8 : 4) == 0 && (uintptr_t)power % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: x is aligned for its element, power for a float");
        frame_power(static_cast<const float*>(x), rows, n, is_complex, L, static_cast<float*>(power), as_stream(stream));
    });
}

int rcfm_tuner_frame_levels(rcfm_tuner_t t, int first, int count, int F, void* scratch, size_t scratch_bytes, void* power,
                            void* stream) {
    return guarded([&] {
        RC_REQUIRE(t && scratch && power, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(F >= 1, RCFM_ERR_ARG, "F must be at least 1");
        RC_REQUIRE((uintptr_t)scratch % 8 == 0 && (uintptr_t)power % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: scratch is aligned for a complex64, power for a float");
        require_channels(first, count, t->nch);
        t->require_readable(first, count, "rcfm_tuner_frame_levels", RCFM_ERR_ARG,
                            "channels of one rcfm_tuner_frame_levels range must share a bandwidth");
        if (count == 0) return;
        const int32_t B = t->bw[first];
        RC_REQUIRE(B % F == 0, RCFM_ERR_ARG, "F does not divide the channels' bandwidth");
        const size_t m = scratch_bytes / (sizeof(float2) * (size_t)B);
        RC_REQUIRE(m >= 1, RCFM_ERR_ARG, "the scratch holds less than one channel");
        hipStream_t s = as_stream(stream);
        float* p = static_cast<float*>(power);
        for (int i = 0; i < count;) {
            const int cnt = (int)std::min<size_t>(m, (size_t)(count - i));
            {
                ArenaScope scope(t->arena);
                t->run(first + i, cnt, static_cast<float2*>(scratch), s);
            }
            frame_power(static_cast<const float*>(scratch), cnt, B, 1, B / F, p + (size_t)i * F, s);
            i += cnt;
        }
    });
}

int rcfm_gate_create(int C, int hang, int lead, const float* ramp_host, int R, rcfm_gate_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1, RCFM_ERR_ARG, "C must be at least 1");
        RC_REQUIRE(hang >= 0 && lead >= 0, RCFM_ERR_ARG, "hang and lead must be at least 0");
        RC_REQUIRE(R >= 0 && R <= kGateMaxRamp, RCFM_ERR_ARG, "ramp length outside 0 .. 2^20");
        RC_REQUIRE(R == 0 || ramp_host != nullptr, RCFM_ERR_ARG, "NULL argument: a ramp of R > 0 samples needs its values");
        for (int i = 0; i < R; ++i) RC_REQUIRE(std::isfinite(ramp_host[i]), RCFM_ERR_ARG, "a ramp element is not finite");
        auto g = std::make_unique<rcfm_gate_s>();
        g->C = C, g->hang = hang, g->lead = lead, g->R = R;
        if (R > 0) g->ramp.upload(ramp_host, sizeof(float) * (size_t)R);
        g->state.reset(g->state_bytes());
        RC_HIP(hipMemset(g->state.get(), 0, g->state_bytes()));
        *out = g.release();
    });
}

int rcfm_gate_run(rcfm_gate_t g, int first, int count, int F, const void* power, const void* open_thr, const void* close_thr,
                  void* frame_mask, void* open_any, void* stream) {
    return guarded([&] {
        RC_REQUIRE(g && power && open_thr && close_thr && frame_mask, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(count >= 0, RCFM_ERR_ARG, "negative channel count");
        RC_REQUIRE(F >= 1 && F <= kGateMaxFrames, RCFM_ERR_ARG, "F outside 1 .. 65535");
        RC_REQUIRE((uintptr_t)power % 4 == 0 && (uintptr_t)open_thr % 4 == 0 && (uintptr_t)close_thr % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: power and the thresholds are aligned for a float");
        RC_REQUIRE(first >= 0 && (int64_t)first + count <= g->C, RCFM_ERR_INDEX, "first .. first + count is outside the gate's channels");
        if (count == 0) return;
        hipStream_t s = as_stream(stream);
        StreamFence::Scope fenced(g->fence, s);
        hipLaunchKernelGGL(k_gate_run, dim3((unsigned)((count + kGateThreads - 1) / kGateThreads)), dim3(kGateThreads), 0, s,
                           g->state.as<int32_t>() + 2 * (size_t)first, static_cast<const float*>(power),
                           static_cast<const float*>(open_thr), static_cast<const float*>(close_thr), count, F, g->hang, g->lead,
                           static_cast<uint8_t*>(frame_mask), static_cast<uint8_t*>(open_any));
        RC_HIP(hipGetLastError());
    });
}

int rcfm_gate_apply(rcfm_gate_t g, const void* frame_mask, int count, int F, int A, int ch, void* audio, void* stream) {
    return guarded([&] {
        RC_REQUIRE(g && frame_mask && audio, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(count >= 0, RCFM_ERR_ARG, "negative channel count");
        RC_REQUIRE(F >= 1 && F <= kGateMaxFrames, RCFM_ERR_ARG, "F outside 1 .. 65535");
        RC_REQUIRE(A >= 1 && A % F == 0, RCFM_ERR_ARG, "F does not divide the audio length A");
        RC_REQUIRE(ch == 1 || ch == 2, RCFM_ERR_ARG, "ch is 1 or 2");
        RC_REQUIRE((uintptr_t)audio % 4 == 0, RCFM_ERR_ARG, "misaligned buffer: audio is aligned for a float");
        const int La = A / F;
        RC_REQUIRE(g->R <= La, RCFM_ERR_ARG, "the gate's ramp is longer than a frame of A / F samples");
        if (count == 0) return;
        hipStream_t s = as_stream(stream);
        const int64_t row = (int64_t)A * ch;
        const bool vec = ((int64_t)La * ch) % 4 == 0 && (uintptr_t)audio % 16 == 0;
        const int64_t items = vec ? row / 4 : row;
        const unsigned bx = (unsigned)((items + kGateThreads - 1) / kGateThreads);
        float* a = static_cast<float*>(audio);
        const uint8_t* m = static_cast<const uint8_t*>(frame_mask);
        for (int c0 = 0; c0 < count; c0 += kMaxGridY) {                 // channels are a grid coordinate
            const dim3 grid(bx, (unsigned)std::min(kMaxGridY, count - c0));
            float* ac = a + (size_t)c0 * row;
            const uint8_t* mc = m + (size_t)c0 * (F + 1);
            if (vec)
                hipLaunchKernelGGL((k_gate_apply<true>), grid, dim3(kGateThreads), 0, s, ac, mc, F, La, ch, row, g->ramp.as<float>(), g->R);
            else
                hipLaunchKernelGGL((k_gate_apply<false>), grid, dim3(kGateThreads), 0, s, ac, mc, F, La, ch, row, g->ramp.as<float>(), g->R);
            RC_HIP(hipGetLastError());
        }
    });
}

int rcfm_gate_reset(rcfm_gate_t g, void* stream) {
    return guarded([&] {
        RC_REQUIRE(g, RCFM_ERR_ARG, "NULL handle");
        RC_HIP(hipMemsetAsync(g->state.get(), 0, g->state_bytes(), as_stream(stream)));
    });
}

int rcfm_gate_get_state(rcfm_gate_t g, int32_t* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(g && state_host, RCFM_ERR_ARG, "NULL argument");
        state_to_host(state_host, g->state.get(), g->state_bytes(), as_stream(stream));
    });
}

int rcfm_gate_set_state(rcfm_gate_t g, const int32_t* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(g && state_host, RCFM_ERR_ARG, "NULL argument");
        state_to_device(g->state.get(), state_host, g->state_bytes(), as_stream(stream));
    });
}

int rcfm_gate_set_fence(rcfm_gate_t g, int on) {
    return guarded([&] {
        RC_REQUIRE(g, RCFM_ERR_ARG, "NULL handle");
        g->fence.arm(on != 0);
    });
}

int rcfm_gate_destroy(rcfm_gate_t g) {
    return guarded([&] { delete g; });
}

}  // extern "C"
