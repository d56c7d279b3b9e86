// The noise floor (include/rcfm.h, "noise floor"): rcfm_rank_filter, a sliding order statistic over the cells of a power
// spectrum with guard cells left out (OS-CFAR); rcfm_floor_run, the same followed by a rise / fall smoothing whose state is
// carried from buffer to buffer, and the mask of the cells over the floor; rcfm_floor_thresholds, the floor of a channel's
// cell times the channel's gain.  No existing kernel is touched: with no floor set none of this is launched.
#include "floor.h"

#include <cmath>
#include <memory>

#include "api_internal.h"

namespace rcfm {

namespace {

// float32 bits -> a key whose unsigned order is the order of include/rcfm.h: by value, -0 below +0, every NaN one key
// above +inf.  No other value maps to that key (it would be the bits 0x7fffffff, a NaN).
__device__ __forceinline__ uint32_t floor_key(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint32_t floor_bits(uint32_t k) {
    if (k == 0xffffffffu) return kFloorNaN;
    return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
}

// Candidates of the cell at LDS word `mid` that lie below `pivot`: the words mid -+ d, guard < d <= half.  EDGE: the
// cell's window is cut by a band end, d reaches dl to the left and dr to the right -- an index test, the words beyond are
// read (they exist) and not counted.  Lane t reads word t + const: adjacent lanes, adjacent banks.
template <bool EDGE>
__device__ __forceinline__ int count_below(const uint32_t* __restrict__ keys, int mid, int guard, int half, int dl, int dr,
                                           uint32_t pivot) {
    int c = 0;
#pragma unroll 4
    for (int d = guard + 1; d <= half; ++d) {
        const uint32_t a = keys[mid - d], b = keys[mid + d];
        if (EDGE) {
            c += (int)(a < pivot && d <= dl) + (int)(b < pivot && d <= dr);
        } else {
            c += (int)(a < pivot) + (int)(b < pivot);
        }
    }
    return c;
}

// The key of rank r among the cell's candidates: the largest key v with fewer than r + 1 candidates below it, built bit by
// bit from the top.  Exact, whatever the values.
template <bool EDGE>
__device__ __forceinline__ uint32_t select_rank(const uint32_t* __restrict__ keys, int mid, int guard, int half, int dl, int dr,
                                                int r) {
    uint32_t v = 0;
    for (int b = 31; b >= 0; --b) {
        const uint32_t trial = v | (1u << b);
        if (count_below<EDGE>(keys, mid, guard, half, dl, dr, trial) <= r) v = trial;
    }
    return v;
}

// Workgroup b owns cells [256 b, 256 b + 256); its LDS holds the keys of cells 256 b - half .. 256 b + 255 + half (0 where
// there is no such cell; those words are never counted).  state == nullptr: out[m] = the rank (rcfm_rank_filter).  Else
// the smoothing of rcfm_floor_run: state, out (the floor) and over as documented there; out and over may be nullptr.
__global__ __launch_bounds__(kFloorThreads) void k_floor(const float* __restrict__ x, int M, int half, int guard, int q,
                                                         float* __restrict__ state, float rise, float fall, float ratio,
                                                         float* __restrict__ out, uint8_t* __restrict__ over) {
#pragma clang fp contract(off)                                      // the smoothing is three roundings, never an fma
    extern __shared__ uint32_t keys[];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kFloorThreads;
    const int words = kFloorThreads + 2 * half;
    for (int i = tid; i < words; i += kFloorThreads) {
        const int64_t g = base - half + i;
        keys[i] = (g >= 0 && g < M) ? floor_key(__float_as_uint(x[g])) : 0u;
    }
    __syncthreads();
    const int64_t m = base + tid;
    if (m >= M) return;
    const int dl = (int)min((int64_t)half, m), dr = (int)min((int64_t)half, (int64_t)M - 1 - m);
    const int cnt = max(dl - guard, 0) + max(dr - guard, 0);
    uint32_t ebits = kFloorNaN;                                     // a cell without a candidate has no estimate
    if (cnt > 0) {
        const int r = (int)(((int64_t)q * (cnt - 1)) / 1000);
        const bool whole = base >= half && base + kFloorThreads - 1 + half <= (int64_t)M - 1;   // (the whole workgroup's)
        const uint32_t k = whole ? select_rank<false>(keys, tid + half, guard, half, dl, dr, r)
                                 : select_rank<true>(keys, tid + half, guard, half, dl, dr, r);
        ebits = floor_bits(k);
    }
    const float e = __uint_as_float(ebits);
    if (state == nullptr) {
        out[m] = e;
        return;
    }
    const float s = state[m];
    float sn;
    if (s != s)
        sn = e;
    else if (e != e)
        sn = s;
    else {
        // __fadd_rn(s, __fmul_rn(a, __fsub_rn(e, s))) in value -- written as plain operators, because the pragma above does
        // not reach into the header's inline functions, whose product and sum the compiler would fuse
        const float d = e - s, step = (e > s ? rise : fall) * d;
        sn = s + step;
    }
    state[m] = sn;
    if (out != nullptr) out[m] = sn;
    if (over != nullptr) over[m] = (uint8_t)(x[m] >= ratio * sn);
}

__global__ __launch_bounds__(kFloorThreads) void k_floor_thresholds(const float* __restrict__ floor, int M,
                                                                    const int32_t* __restrict__ cell,
                                                                    const float* __restrict__ gain, int count,
                                                                    float* __restrict__ thr) {
    const int i = blockIdx.x * kFloorThreads + threadIdx.x;
    if (i >= count) return;
    const int32_t c = cell[i];
    thr[i] = (c >= 0 && c < M) ? __fmul_rn(floor[c], gain[i]) : __uint_as_float(kFloorNaN);
}

void require_window(int64_t M, int half, int guard, int q) {
    RC_REQUIRE(half >= 1 && half <= kFloorMaxHalf, RCFM_ERR_ARG, "half outside 1 .. 4096");
    RC_REQUIRE(guard >= 0 && guard <= half - 1, RCFM_ERR_ARG, "guard outside 0 .. half - 1");
    RC_REQUIRE(q >= 0 && q <= 1000, RCFM_ERR_ARG, "q outside 0 .. 1000");
    RC_REQUIRE(M >= (int64_t)guard + 2, RCFM_ERR_ARG, "M is below guard + 2: a cell would have no candidate");
    RC_REQUIRE(M <= kFloorMaxCells, RCFM_ERR_ARG, "M is above 2^30");
}

void launch_floor(const float* x, int64_t M, int half, int guard, int q, float* state, float rise, float fall, float ratio,
                  float* out, uint8_t* over, hipStream_t s) {
    const unsigned grid = (unsigned)((M + kFloorThreads - 1) / kFloorThreads);
    const size_t lds = sizeof(uint32_t) * (size_t)(kFloorThreads + 2 * half);
    hipLaunchKernelGGL(k_floor, dim3(grid), dim3(kFloorThreads), lds, s, x, (int)M, half, guard, q, state, rise, fall, ratio,
                       out, over);
    RC_HIP(hipGetLastError());
}

}  // namespace

}  // namespace rcfm

using namespace rcfm;

struct rcfm_floor_s {
    int64_t M = 0;
    int half = 0, guard = 0, q = 0;
    float rise = 1.f, fall = 1.f;
    DeviceBuffer state;                // float32 [M]; NaN: not primed
    StreamFence fence;                 // rcfm_floor_set_fence
    size_t state_bytes() const { return (size_t)M * sizeof(float); }
};

extern "C" {

int rcfm_rank_filter(const void* x, int64_t M, int half, int guard, int q, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(x && out, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(x != out, RCFM_ERR_ARG, "out must not be x: every cell reads its neighbours");
        require_window(M, half, guard, q);
        RC_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)out % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: x and out are aligned for a float");
        launch_floor(static_cast<const float*>(x), M, half, guard, q, nullptr, 1.f, 1.f, 0.f, static_cast<float*>(out), nullptr,
                     as_stream(stream));
    });
}

int rcfm_floor_create(int64_t M, int half, int guard, int q, float rise, float fall, rcfm_floor_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "NULL argument");
        require_window(M, half, guard, q);
        RC_REQUIRE(std::isfinite(rise) && rise > 0.f && rise <= 1.f, RCFM_ERR_ARG, "rise is not in (0, 1]");
        RC_REQUIRE(std::isfinite(fall) && fall > 0.f && fall <= 1.f, RCFM_ERR_ARG, "fall is not in (0, 1]");
        auto h = std::make_unique<rcfm_floor_s>();
        h->M = M, h->half = half, h->guard = guard, h->q = q, h->rise = rise, h->fall = fall;
        h->state.reset(h->state_bytes());
        RC_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(h->state.get()), (int)kFloorNaN, (size_t)M));
        *out = h.release();
    });
}

int rcfm_floor_run(rcfm_floor_t h, const void* power, float ratio, void* floor, void* over, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h && power, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(floor || over, RCFM_ERR_ARG, "NULL argument: floor and over are both NULL");
        RC_REQUIRE(power != floor, RCFM_ERR_ARG, "floor must not be power: every cell reads its neighbours");
        RC_REQUIRE(!std::isnan(ratio), RCFM_ERR_ARG, "ratio is NaN");
        RC_REQUIRE((uintptr_t)power % 4 == 0 && (uintptr_t)floor % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: power and floor are aligned for a float");
        hipStream_t s = as_stream(stream);
        StreamFence::Scope fenced(h->fence, s);
        launch_floor(static_cast<const float*>(power), h->M, h->half, h->guard, h->q, h->state.as<float>(), h->rise, h->fall,
                     ratio, static_cast<float*>(floor), static_cast<uint8_t*>(over), s);
    });
}

int rcfm_floor_thresholds(const void* floor, int64_t M, const void* cell, const void* gain, int count, void* thr, void* stream) {
    return guarded([&] {
        RC_REQUIRE(floor && cell && gain && thr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(M >= 1 && M <= kFloorMaxCells, RCFM_ERR_ARG, "M outside 1 .. 2^30");
        RC_REQUIRE(count >= 0, RCFM_ERR_ARG, "negative channel count");
        RC_REQUIRE((uintptr_t)floor % 4 == 0 && (uintptr_t)cell % 4 == 0 && (uintptr_t)gain % 4 == 0 && (uintptr_t)thr % 4 == 0,
                   RCFM_ERR_ARG, "misaligned buffer: floor, cell, gain and thr are aligned for four bytes");
        if (count == 0) return;
        hipLaunchKernelGGL(k_floor_thresholds, dim3((unsigned)((count + kFloorThreads - 1) / kFloorThreads)), dim3(kFloorThreads),
                           0, as_stream(stream), static_cast<const float*>(floor), (int)M, static_cast<const int32_t*>(cell),
                           static_cast<const float*>(gain), count, static_cast<float*>(thr));
        RC_HIP(hipGetLastError());
    });
}

int rcfm_floor_reset(rcfm_floor_t h, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h, RCFM_ERR_ARG, "NULL handle");
        RC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->state.get()), (int)kFloorNaN, (size_t)h->M, as_stream(stream)));
    });
}

int rcfm_floor_get_state(rcfm_floor_t h, float* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h && state_host, RCFM_ERR_ARG, "NULL argument");
        state_to_host(state_host, h->state.get(), h->state_bytes(), as_stream(stream));
    });
}

int rcfm_floor_set_state(rcfm_floor_t h, const float* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h && state_host, RCFM_ERR_ARG, "NULL argument");
        state_to_device(h->state.get(), state_host, h->state_bytes(), as_stream(stream));
    });
}

int rcfm_floor_set_fence(rcfm_floor_t h, int on) {
    return guarded([&] {
        RC_REQUIRE(h, RCFM_ERR_ARG, "NULL handle");
        h->fence.arm(on != 0);
    });
}

int rcfm_floor_destroy(rcfm_floor_t h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
