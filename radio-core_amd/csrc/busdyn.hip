// Bus dynamics (include/rcfm.h, "bus dynamics"): a look-ahead peak limiter with a ducking side-chain behind rcfm_mix_run.
// Three launches per run on the caller's stream: the block peaks of every bus (exact maxima, any order), the gain knots (one
// wave per bus walks its blocks in order: a min of an affine step, which cannot be re-associated), and the apply, which reads every
// sample L behind, interpolates the gain between two knots, multiplies, clamps and stores.  The tail of L samples lives in
// two slots; a run reads one and writes the other, so no workgroup overwrites what another still reads.  Which is which
// is a run counter in device memory, stepped by the knot kernel -- the one writer, between the two launches that read it.  No atomics, no
// existing kernel touched: without a handle none of this is launched.
#pragma clang fp contract(off)             // every product, sum and quotient below is one rounding of its own, never an fma

#include "busdyn.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "common.h"

namespace rcfm {

namespace {

// The maximum of the definition: a NaN v never wins, and p never is one (it starts at +0).
__device__ __forceinline__ float max_nn(float v, float p) { return v > p ? v : p; }

__device__ __forceinline__ float wave_max(float p) {
    for (int d = 32; d > 0; d >>= 1) p = max_nn(__shfl_xor(p, d, 64), p);     // every lane ends with the same maximum
    return p;
}

// P[m][j], j = 0 .. B: the peak of bus m's tail (j = 0; slot epoch & 1 of the two) and of block j - 1 of its row, [e, min(e + L, A)) from e = (j - 1) L.
// One wave per peak, four peaks per workgroup; VEC: 16-byte loads ((L ch) % 4 == 0, (A ch) % 4 == 0 and a 16-byte base, so
// every block starts on a vector and holds whole vectors), else 4-byte loads.  A maximum is exact in any order.
template <bool VEC>
__global__ __launch_bounds__(kBusdynThreads) void k_busdyn_peaks(const float* __restrict__ in, const float* __restrict__ tails,
                                                                 const uint32_t* __restrict__ epoch, int M, int A, int L, int ch,
                                                                 int B, float* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kBusdynThreads / 64) + (int)(threadIdx.x >> 6));
    const int m = blockIdx.y;
    if (j > B) return;
    const float* src;
    int n;                                 // floats of this peak: at most 2048 x 2
    if (j == 0) {
        src = tails + ((size_t)(epoch[0] & 1u) * M + m) * L * ch;       // the slot the previous run wrote
        n = L * ch;
    } else {
        const int64_t e0 = (int64_t)(j - 1) * L;
        src = in + ((size_t)m * A + (size_t)e0) * ch;
        n = (A - e0 < L ? (int)(A - e0) : L) * ch;
    }
    float p = 0.f;
    if (VEC) {
        for (int f = 4 * lane; f < n; f += 256) {
            const float4 v = *reinterpret_cast<const float4*>(src + f);
            p = max_nn(fabsf(v.x), p), p = max_nn(fabsf(v.y), p), p = max_nn(fabsf(v.z), p), p = max_nn(fabsf(v.w), p);
        }
    } else {
        for (int f = lane; f < n; f += 64) p = max_nn(fabsf(src[f]), p);
    }
    p = wave_max(p);
    if (lane == 0) P[(size_t)m * (B + 1) + j] = p;
}

// Wave m walks the knots of bus m: H[m][0] = the state, H[m][b] = min(T_b, release step), b = 1 .. B, and leaves h[B] and
// the hang counter as the new state.  64 knots at a time: lane l loads the peaks of knot b0 + l and computes what does not
// depend on the chain -- T, min(T, d), whether the key bus is active -- and then every lane walks the 64 knots in order, the
// figures of knot i coming by v_readlane from lane i: per knot one subtract, one product, one sum and one compare, no load.
// Bus 0's wave steps the run counter.
// (One thread per bus that loaded its peaks as it went took 30 us for 125 knots: the loads' round trips, not the chain.)
__global__ __launch_bounds__(kBusdynKnotThreads) void k_busdyn_knots(const float* __restrict__ P, int B, float c, float k,
                                                                     const int32_t* __restrict__ key, const float* __restrict__ depth,
                                                                     const float* __restrict__ thr, const int32_t* __restrict__ hold,
                                                                     float* __restrict__ hstate, int32_t* __restrict__ hang_state,
                                                                     const uint8_t* __restrict__ open_in, uint8_t* __restrict__ open_out,
                                                                     float* __restrict__ H, uint32_t* __restrict__ epoch) {
#pragma clang fp contract(off)
    const int m = blockIdx.x, lane = threadIdx.x;
    const size_t S = (size_t)B + 1;
    float h = hstate[m];
    int hang = hang_state[m];
    const int km = key != nullptr ? key[m] : -1;
    float d = 1.f, t = 0.f;
    int hd = 0;
    if (km >= 0) d = depth[m], t = thr[m], hd = hold[m];
    const float* Pm = P + (size_t)m * S;
    const float* Pk = P + (size_t)(km >= 0 ? km : m) * S;
    float* Hm = H + (size_t)m * S;
    const float tail_peak = Pm[0];
    if (lane == 0) Hm[0] = h;
    for (int b0 = 1; b0 <= B; b0 += 64) {
        const int b = b0 + lane;
        float T = 1.f, Td = 1.f;
        bool hit = false;
        if (b <= B) {
            const float Q = max_nn(Pm[b], Pm[b - 1]);
            T = Q > c ? c / Q : 1.f;
            if (km >= 0) {
                hit = max_nn(Pk[b], Pk[b - 1]) > t;
                Td = d < T ? d : T;
            }
        }
        const uint64_t hits = __ballot(hit);
        const int n = B - b0 + 1 < 64 ? B - b0 + 1 : 64;
        float mine = 0.f;
        for (int i = 0; i < n; ++i) {
            float Ti = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(T), i));
            if (km >= 0) {
                bool on = true;
                if ((hits >> i) & 1)
                    hang = hd;
                else if (hang > 0)
                    --hang;
                else
                    on = false;
                if (on) Ti = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Td), i));
            }
            const float r = h + ((1.f - h) * k);
            h = Ti < r ? Ti : r;
            if (lane == i) mine = h;
        }
        if (b <= B) Hm[b] = mine;
    }
    if (lane == 0) {
        hstate[m] = h;
        hang_state[m] = hang;
        if (open_out != nullptr) open_out[m] = (uint8_t)(open_in == nullptr || open_in[m] != 0 || tail_peak > 0.f);
        if (m == 0) epoch[0] = epoch[0] + 1u;      // the peaks read slot epoch & 1; the apply reads it as (epoch - 1) & 1 and writes the other
    }
}

// One thread per item of bus m's output row: VEC, four floats (16-byte loads and stores: 16-byte bases, (A ch) % 4 == 0 and
// (L ch) % 4 == 0, so a vector lies in one block and on one side of the seam between tail and row), else one float.  Float f
// is leg f % ch of sample n = f / ch, whose source lies L samples behind: in the old tail for n < L, else in the row.
// Workgroups x >= nbx write the new tail, the last L samples of tail ++ row, into the other slot: no workgroup of this launch
// reads that one.
template <bool VEC>
__global__ __launch_bounds__(kBusdynThreads) void k_busdyn_apply(const float* __restrict__ in, float* tails,
                                                                 const uint32_t* __restrict__ epoch, const float* __restrict__ H,
                                                                 int M, int A, int L, int ch, int B, int nbx, float c,
                                                                 float* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int W = VEC ? 4 : 1;
    const int m = blockIdx.y;
    const int64_t row = (int64_t)A * ch, lag = (int64_t)L * ch;
    const uint32_t run = epoch[0];             // this run's knots have stepped it: the old tail is slot (run - 1) & 1
    const float* x_row = in + (size_t)m * (size_t)row;
    const float* x_tail = tails + ((size_t)((run - 1u) & 1u) * M + m) * (size_t)lag;
    float* tail_new = tails + (size_t)(run & 1u) * M * (size_t)lag;
    if ((int)blockIdx.x < nbx) {
        const int64_t f = ((int64_t)blockIdx.x * kBusdynThreads + threadIdx.x) * W;
        if (f >= row) return;
        const int n = (int)(ch == 2 ? f >> 1 : f);
        const int j = n / L, i = n - j * L;
        const float len = (float)(A - j * L < L ? A - j * L : L);
        const float* src = f < lag ? x_tail + f : x_row + (f - lag);
        const float h0 = H[(size_t)m * (B + 1) + j], h1 = H[(size_t)m * (B + 1) + j + 1];
        const float dh = h1 - h0;
        float x[W], y[W];
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(src);
            x[0] = v.x, x[W / 4] = v.y, x[W / 2] = v.z, x[W - 1] = v.w;
        } else {
            x[0] = *src;
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const float w = (float)(i + (ch == 2 ? e >> 1 : e) + 1) / len;
            const float g = h0 + (dh * w);
            const float v = x[e] * g;
            y[e] = v > c ? c : (v < -c ? -c : v);
        }
        float* dst = out + (size_t)m * (size_t)row + f;
        if (VEC)
            *reinterpret_cast<float4*>(dst) = make_float4(y[0], y[W / 4], y[W / 2], y[W - 1]);
        else
            *dst = y[0];
    } else {
        const int64_t f = ((int64_t)((int)blockIdx.x - nbx) * kBusdynThreads + threadIdx.x) * W;
        if (f >= lag) return;
        const int64_t e = row + f;         // float e of tail ++ row
        const float* src = e < lag ? x_tail + e : x_row + (e - lag);
        float* dst = tail_new + (size_t)m * (size_t)lag + f;
        if (VEC)
            *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
        else
            *dst = *src;
    }
}

__global__ void k_busdyn_ones(float* __restrict__ h, int M) {
    const int m = (int)blockIdx.x * kBusdynKnotThreads + (int)threadIdx.x;
    if (m < M) h[m] = 1.f;
}

}  // namespace

}  // namespace rcfm

using namespace rcfm;

struct rcfm_busdyn_s {
    int M = 0, ch = 0, L = 0, A_max = 0;
    float c = 0.f, k = 0.f;
    bool duck = false;
    DeviceBuffer tail, hval, hang;         // float32 [2][M][L][ch]; float32 [M]; int32 [M]
    DeviceBuffer epoch;                    // uint32 [1]: the runs so far; the tail is slot epoch & 1
    DeviceBuffer peaks, knots;             // scratch, float32 [M][B + 1] of a run, each sized for B = ceil(A_max / L)
    DeviceBuffer key, depth, thr, hold;
    StreamFence fence;                     // rcfm_busdyn_set_fence
    size_t tail_floats() const { return (size_t)M * L * ch; }
    unsigned knot_grid() const { return (unsigned)((M + kBusdynKnotThreads - 1) / kBusdynKnotThreads); }   // of k_busdyn_ones
    void rest(hipStream_t s) {
        RC_HIP(hipMemsetAsync(tail.get(), 0, 2 * tail_floats() * sizeof(float), s));
        RC_HIP(hipMemsetAsync(hang.get(), 0, (size_t)M * sizeof(int32_t), s));
        RC_HIP(hipMemsetAsync(epoch.get(), 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_busdyn_ones, dim3(knot_grid()), dim3(kBusdynKnotThreads), 0, s, hval.as<float>(), M);
        RC_HIP(hipGetLastError());
    }
};

extern "C" {

int rcfm_busdyn_create(int M, int ch, int L, int A_max, float ceiling, float release_k, const int32_t* key_host,
                       const float* depth_host, const float* thr_host, const int32_t* hold_host, rcfm_busdyn_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(M >= 1 && M <= kBusdynMaxBuses, RCFM_ERR_ARG, "M outside 1 .. 1024");
        RC_REQUIRE(ch == 1 || ch == 2, RCFM_ERR_ARG, "ch outside {1, 2}");
        RC_REQUIRE(L >= kBusdynMinBlock && L <= kBusdynMaxBlock, RCFM_ERR_ARG, "L outside 8 .. 2048");
        RC_REQUIRE(A_max >= 1 && A_max <= kBusdynMaxLength, RCFM_ERR_ARG, "A_max outside 1 .. 2^30");
        RC_REQUIRE(std::isfinite(ceiling) && ceiling > 0.f, RCFM_ERR_ARG, "the ceiling is not finite and above 0");
        RC_REQUIRE(release_k > 0.f && release_k <= 1.f, RCFM_ERR_ARG, "release_k outside (0, 1]");
        const bool duck = key_host != nullptr;
        if (duck) {
            RC_REQUIRE(depth_host && thr_host && hold_host, RCFM_ERR_ARG, "NULL argument: a key table needs depth, thr and hold");
            for (int m = 0; m < M; ++m) {
                RC_REQUIRE(key_host[m] >= -1 && key_host[m] < M, RCFM_ERR_ARG, "a key is outside -1 .. M - 1");
                RC_REQUIRE(key_host[m] != m, RCFM_ERR_ARG, "a bus is its own key");
                RC_REQUIRE(depth_host[m] > 0.f && depth_host[m] <= 1.f, RCFM_ERR_ARG, "a depth is outside (0, 1]");
                RC_REQUIRE(thr_host[m] >= 0.f, RCFM_ERR_ARG, "a threshold is below 0 or not a number");
                RC_REQUIRE(hold_host[m] >= 0 && hold_host[m] <= kBusdynMaxHold, RCFM_ERR_ARG, "a hold is outside 0 .. 2^15");
            }
        }
        auto h = std::make_unique<rcfm_busdyn_s>();
        h->M = M, h->ch = ch, h->L = L, h->A_max = A_max, h->c = ceiling, h->k = release_k, h->duck = duck;
        if (duck) {
            h->key.upload(key_host, sizeof(int32_t) * (size_t)M);
            h->depth.upload(depth_host, sizeof(float) * (size_t)M);
            h->thr.upload(thr_host, sizeof(float) * (size_t)M);
            h->hold.upload(hold_host, sizeof(int32_t) * (size_t)M);
        }
        const size_t knots = ((size_t)(A_max + L - 1) / L + 1) * (size_t)M;
        h->tail.reset(2 * h->tail_floats() * sizeof(float));
        h->hval.reset((size_t)M * sizeof(float));
        h->hang.reset((size_t)M * sizeof(int32_t));
        h->epoch.reset(sizeof(uint32_t));
        h->peaks.reset(knots * sizeof(float));
        h->knots.reset(knots * sizeof(float));
        h->rest(nullptr);
        RC_HIP(hipStreamSynchronize(nullptr));
        *out = h.release();
    });
}

int rcfm_busdyn_run(rcfm_busdyn_t h, int A, const void* in, const void* bus_open_in, void* out, void* bus_open_out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h && in && out, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(A >= 1, RCFM_ERR_ARG, "A below 1");
        const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
        RC_REQUIRE(i0 % 4 == 0 && o0 % 4 == 0, RCFM_ERR_ARG, "misaligned buffer: in and out are aligned for a float");
        RC_REQUIRE(i0 != o0, RCFM_ERR_ARG, "out overlaps in");
        RC_REQUIRE(A <= h->A_max, RCFM_ERR_ARG, "A above the handle's A_max");
        const int M = h->M, ch = h->ch, L = h->L;
        const size_t bytes = sizeof(float) * (size_t)M * (size_t)A * (size_t)ch;
        RC_REQUIRE(i0 + bytes <= o0 || o0 + bytes <= i0, RCFM_ERR_ARG, "out overlaps in");
        hipStream_t s = as_stream(stream);
        StreamFence::Scope fenced(h->fence, s);
        const int B = (A + L - 1) / L;
        const int64_t row = (int64_t)A * ch, lag = (int64_t)L * ch;
        const float* x = static_cast<const float*>(in);
        float* tails = h->tail.as<float>();
        uint32_t* epoch = h->epoch.as<uint32_t>();
        float* P = h->peaks.as<float>();
        float* H = h->knots.as<float>();
        const dim3 pgrid((unsigned)((B + 1 + kBusdynThreads / 64 - 1) / (kBusdynThreads / 64)), (unsigned)M);
        if (i0 % 16 == 0 && row % 4 == 0 && lag % 4 == 0)
            hipLaunchKernelGGL((k_busdyn_peaks<true>), pgrid, dim3(kBusdynThreads), 0, s, x, tails, epoch, M, A, L, ch, B, P);
        else
            hipLaunchKernelGGL((k_busdyn_peaks<false>), pgrid, dim3(kBusdynThreads), 0, s, x, tails, epoch, M, A, L, ch, B, P);
        RC_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_busdyn_knots, dim3((unsigned)M), dim3(kBusdynKnotThreads), 0, s, P, B, h->c, h->k,
                           h->duck ? h->key.as<int32_t>() : nullptr, h->depth.as<float>(), h->thr.as<float>(), h->hold.as<int32_t>(),
                           h->hval.as<float>(), h->hang.as<int32_t>(), static_cast<const uint8_t*>(bus_open_in),
                           static_cast<uint8_t*>(bus_open_out), H, epoch);
        RC_HIP(hipGetLastError());
        const bool vec = i0 % 16 == 0 && o0 % 16 == 0 && row % 4 == 0 && lag % 4 == 0;
        const int64_t per = (int64_t)kBusdynThreads * (vec ? 4 : 1);      // floats per workgroup
        const int nbx = (int)((row + per - 1) / per);
        const dim3 agrid((unsigned)(nbx + (int)((lag + per - 1) / per)), (unsigned)M);
        if (vec)
            hipLaunchKernelGGL((k_busdyn_apply<true>), agrid, dim3(kBusdynThreads), 0, s, x, tails, epoch, H, M, A, L, ch, B, nbx,
                               h->c, static_cast<float*>(out));
        else
            hipLaunchKernelGGL((k_busdyn_apply<false>), agrid, dim3(kBusdynThreads), 0, s, x, tails, epoch, H, M, A, L, ch, B, nbx,
                               h->c, static_cast<float*>(out));
        RC_HIP(hipGetLastError());
    });
}

int rcfm_busdyn_reset(rcfm_busdyn_t h, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h, RCFM_ERR_ARG, "NULL handle");
        h->rest(as_stream(stream));
    });
}

int rcfm_busdyn_set_fence(rcfm_busdyn_t h, int on) {
    return guarded([&] {
        RC_REQUIRE(h, RCFM_ERR_ARG, "NULL handle");
        h->fence.arm(on != 0);
    });
}

int rcfm_busdyn_state(rcfm_busdyn_t h, float* tail_host, float* hval_host, int32_t* hang_host) {
    return guarded([&] {
        RC_REQUIRE(h, RCFM_ERR_ARG, "NULL handle");
        RC_HIP(hipDeviceSynchronize());
        uint32_t runs = 0;
        RC_HIP(hipMemcpy(&runs, h->epoch.get(), sizeof(runs), hipMemcpyDeviceToHost));
        const float* tail = h->tail.as<float>() + (size_t)(runs & 1u) * h->tail_floats();
        if (tail_host) RC_HIP(hipMemcpy(tail_host, tail, h->tail_floats() * sizeof(float), hipMemcpyDeviceToHost));
        if (hval_host) RC_HIP(hipMemcpy(hval_host, h->hval.get(), (size_t)h->M * sizeof(float), hipMemcpyDeviceToHost));
        if (hang_host) RC_HIP(hipMemcpy(hang_host, h->hang.get(), (size_t)h->M * sizeof(int32_t), hipMemcpyDeviceToHost));
    });
}

int rcfm_busdyn_destroy(rcfm_busdyn_t h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
