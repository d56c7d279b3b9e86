// Audio buses (include/rcfm.h, "audio buses"): rcfm_mix_run adds the open channels' audio rows into a few bus rows, every
// route at its own pair of gains, in ONE summation order that the route list alone fixes: segments of 16 routes, each summed
// from +0 in route order, the segment sums added from +0 in segment order.  No atomics, no existing kernel touched: with no
// mixer set none of this is launched.
#pragma clang fp contract(off)             // every product and every sum below is one rounding of its own, never an fma

#include "mix.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "common.h"

namespace rcfm {

namespace {

// __fmul_rn / __fadd_rn in value, as plain operators under the pragma above (it does not reach into the header's inline
// functions, whose product and sum the compiler would be free to fuse).
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// The four samples a lane holds of its workgroup's tile, as positions in the tile: VIN, 4 lane + i (one or two 16-byte
// loads per row); else 64 i + lane (adjacent lanes, adjacent floats: 4-byte loads that coalesce).
template <bool VIN>
__device__ __forceinline__ int tile_pos(int lane, int i) {
    return VIN ? 4 * lane + i : 64 * i + lane;
}

// x[i][leg] = the lane's four samples of one row (A samples of CH_IN legs, tile from sample a0); 0 beyond the row's end.
template <int CH_IN, bool VIN>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int a0, int A, int lane, float (&x)[4][CH_IN]) {
    if (VIN) {
        // (A CH_IN) % 4 == 0 and a 16-byte base: every vector lies whole inside the row or whole outside it
        const int64_t f0 = ((int64_t)a0 + 4 * lane) * CH_IN, len = (int64_t)A * CH_IN;
        float4 v[CH_IN];
#pragma unroll
        for (int k = 0; k < CH_IN; ++k)
            v[k] = f0 + 4 * k < len ? *reinterpret_cast<const float4*>(row + f0 + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (CH_IN == 1) {
            x[0][0] = v[0].x, x[1][0] = v[0].y, x[2][0] = v[0].z, x[3][0] = v[0].w;
        } else {
            x[0][0] = v[0].x, x[0][CH_IN - 1] = v[0].y, x[1][0] = v[0].z, x[1][CH_IN - 1] = v[0].w;
            x[2][0] = v[CH_IN - 1].x, x[2][CH_IN - 1] = v[CH_IN - 1].y, x[3][0] = v[CH_IN - 1].z, x[3][CH_IN - 1] = v[CH_IN - 1].w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t a = (int64_t)a0 + 64 * i + lane;
#pragma unroll
            for (int k = 0; k < CH_IN; ++k) x[i][k] = a < A ? row[a * CH_IN + k] : 0.f;
        }
    }
}

// Workgroup (blockIdx.x, blockIdx.y): samples [256 blockIdx.x, + 256) of bus blockIdx.y.  Per round its kMixWaves waves take
// as many consecutive segments of the bus, one each: lanes 0 .. 15 fetch the segment's routes (channel, mask byte, gains), a
// ballot makes the open ones a wave-uniform bit set, and the wave walks that set in route order, kMixBatch routes at a time
// -- the row loads of all of them are issued, then their terms are added in order.  A closed route's row is never read.  The
// segment sums go to LDS; thread t < 256 CH_OUT then adds the round's sums, in segment order, to float t of the tile.
// active / bus_open: the open routes of the bus, counted from the same ballots, written by the bus's first workgroup.
// With one bus over all 760 airband channels a launch is 32 workgroups, and what it takes is the chain of load round trips
// each wave walks: 16 waves (three rounds for 48 segments) and batches of 8 measured 14.8 us there, 8 waves and batches of
// 4 measured 27.7 us.
template <int CH_IN, int CH_OUT, bool VIN, bool VOUT>
__global__ __launch_bounds__(kMixThreads) void k_mix(const float* __restrict__ audio, const uint8_t* __restrict__ open, int first,
                                                     int A, const int32_t* __restrict__ bus_start,
                                                     const int32_t* __restrict__ chan, const float2* __restrict__ gain,
                                                     float* __restrict__ out, int32_t* __restrict__ active,
                                                     uint8_t* __restrict__ bus_open) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float part[kMixWaves][kMixTile * CH_OUT];
    __shared__ int n_open[kMixWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = blockIdx.y;
    const int r0 = bus_start[m], r1 = bus_start[m + 1];
    const int K = (r1 - r0 + kMixSegment - 1) / kMixSegment;
    const int a0 = (int)blockIdx.x * kMixTile;
    const size_t row_in = (size_t)A * CH_IN;
    float acc = 0.f;
    int cnt = 0;
    for (int kb = 0; kb < K; kb += kMixWaves) {
        const int k = kb + w;
        if (k < K) {
            const int j0 = r0 + kMixSegment * k;
            int cj = 0;
            float gl = 0.f, gr = 0.f;
            bool oj = false;
            if (lane < kMixSegment && j0 + lane < r1) {
                cj = chan[j0 + lane] - first;
                const float2 g = gain[j0 + lane];
                gl = g.x, gr = g.y;
                oj = open == nullptr || open[cj] != 0;
            }
            uint32_t bits = (uint32_t)__ballot(oj);
            cnt += __popc(bits);
            float s[4][CH_OUT];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < CH_OUT; ++c) s[i][c] = 0.f;
            while (bits != 0) {
                float x[kMixBatch][4][CH_IN];
                float g0[kMixBatch], g1[kMixBatch];
                bool has[kMixBatch];
#pragma unroll
                for (int u = 0; u < kMixBatch; ++u) {
                    has[u] = bits != 0;
                    if (has[u]) {
                        const int q = __builtin_ctz(bits);
                        bits &= bits - 1;
                        const int c = __builtin_amdgcn_readlane(cj, q);
                        g0[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gl), q));
                        g1[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gr), q));
                        load_row<CH_IN, VIN>(audio + (size_t)c * row_in, a0, A, lane, x[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < kMixBatch; ++u) {
                    if (has[u]) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float tl = mul_rn(g0[u], x[u][i][0]), tr = mul_rn(g1[u], x[u][i][CH_IN - 1]);
                            if (CH_OUT == 2) {
                                s[i][0] = add_rn(s[i][0], tl);
                                s[i][CH_OUT - 1] = add_rn(s[i][CH_OUT - 1], tr);
                            } else {
                                s[i][0] = add_rn(s[i][0], CH_IN == 2 ? add_rn(tl, tr) : tl);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < CH_OUT; ++c) part[w][tile_pos<VIN>(lane, i) * CH_OUT + c] = s[i][c];
        }
        __syncthreads();
        if (tid < kMixTile * CH_OUT) {
            const int nw = min(kMixWaves, K - kb);
            for (int ww = 0; ww < nw; ++ww) acc = add_rn(acc, part[ww][tid]);
        }
        __syncthreads();
    }
    const int64_t len = (int64_t)A * CH_OUT, f0 = (int64_t)a0 * CH_OUT;
    float* o = out + (size_t)m * (size_t)len;
    if (VOUT) {
        // (A CH_OUT) % 4 == 0 and a 16-byte base: the tile's floats go out as whole 16-byte vectors
        if (tid < kMixTile * CH_OUT) part[0][tid] = acc;
        __syncthreads();
        if (tid < kMixTile * CH_OUT / 4 && f0 + 4 * tid < len)
            *reinterpret_cast<float4*>(o + f0 + 4 * tid) = *reinterpret_cast<const float4*>(&part[0][4 * tid]);
    } else {
        if (tid < kMixTile * CH_OUT && f0 + tid < len) o[f0 + tid] = acc;
    }
    if (blockIdx.x == 0 && (active != nullptr || bus_open != nullptr)) {
        if (lane == 0) n_open[w] = cnt;
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int ww = 0; ww < kMixWaves; ++ww) n += n_open[ww];
            if (active != nullptr) active[m] = n;
            if (bus_open != nullptr) bus_open[m] = (uint8_t)(n > 0);
        }
    }
}

template <int CH_IN, int CH_OUT>
void launch_mix(bool vin, bool vout, dim3 grid, hipStream_t s, const float* audio, const uint8_t* open, int first, int A,
                const int32_t* bus_start, const int32_t* chan, const float2* gain, float* out, int32_t* active,
                uint8_t* bus_open) {
    const dim3 block(kMixThreads);
    if (vin && vout)
        hipLaunchKernelGGL((k_mix<CH_IN, CH_OUT, true, true>), grid, block, 0, s, audio, open, first, A, bus_start, chan, gain, out,
                           active, bus_open);
    else if (vin)
        hipLaunchKernelGGL((k_mix<CH_IN, CH_OUT, true, false>), grid, block, 0, s, audio, open, first, A, bus_start, chan, gain, out,
                           active, bus_open);
    else if (vout)
        hipLaunchKernelGGL((k_mix<CH_IN, CH_OUT, false, true>), grid, block, 0, s, audio, open, first, A, bus_start, chan, gain, out,
                           active, bus_open);
    else
        hipLaunchKernelGGL((k_mix<CH_IN, CH_OUT, false, false>), grid, block, 0, s, audio, open, first, A, bus_start, chan, gain, out,
                           active, bus_open);
    RC_HIP(hipGetLastError());
}

}  // namespace

}  // namespace rcfm

using namespace rcfm;

struct rcfm_mix_s {
    int M = 0, ch_out = 0;
    int32_t lo = 0, hi = -1;               // the least and the greatest channel any route names (hi < lo: no route)
    // the tables on the host, as rcfm_mix_create received them, and on the device: plain hipMalloc, never an arena's
    std::vector<int32_t> bus_start, chan;
    std::vector<float> gain;
    DeviceBuffer bus_start_dev, chan_dev, gain_dev;
};

extern "C" {

int rcfm_mix_create(int M, const int32_t* bus_start_host, const int32_t* route_channel_host, const float* route_gain_host,
                    int ch_out, rcfm_mix_t* out) {
    return guarded([&] {
        RC_REQUIRE(bus_start_host && route_channel_host && route_gain_host && out, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(M >= 1 && M <= kMixMaxBuses, RCFM_ERR_ARG, "M outside 1 .. 1024");
        RC_REQUIRE(ch_out == 1 || ch_out == 2, RCFM_ERR_ARG, "ch_out outside {1, 2}");
        RC_REQUIRE(bus_start_host[0] == 0, RCFM_ERR_ARG, "bus_start[0] is not 0");
        for (int m = 0; m < M; ++m) {
            const int64_t n = (int64_t)bus_start_host[m + 1] - bus_start_host[m];
            RC_REQUIRE(n >= 0, RCFM_ERR_ARG, "bus_start is not monotone");
            RC_REQUIRE(n <= kMixMaxBusRoutes, RCFM_ERR_ARG, "a bus has more than 65535 routes");
            RC_REQUIRE(bus_start_host[m + 1] <= kMixMaxRoutes, RCFM_ERR_ARG, "more than 2^20 routes");
        }
        const int R = bus_start_host[M];
        auto h = std::make_unique<rcfm_mix_s>();
        h->M = M, h->ch_out = ch_out;
        h->bus_start.assign(bus_start_host, bus_start_host + M + 1);
        h->chan.assign(route_channel_host, route_channel_host + R);
        h->gain.assign(route_gain_host, route_gain_host + 2 * (size_t)R);
        for (int j = 0; j < R; ++j) {
            RC_REQUIRE(h->chan[j] >= 0, RCFM_ERR_ARG, "negative channel index");
            RC_REQUIRE(std::isfinite(h->gain[2 * j]) && std::isfinite(h->gain[2 * j + 1]), RCFM_ERR_ARG, "a gain is not finite");
        }
        std::vector<int32_t> sorted;
        for (int m = 0; m < M; ++m) {
            sorted.assign(h->chan.begin() + h->bus_start[m], h->chan.begin() + h->bus_start[m + 1]);
            std::sort(sorted.begin(), sorted.end());
            RC_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), RCFM_ERR_ARG,
                       "a channel appears twice in one bus");
        }
        if (R > 0) {
            const auto mm = std::minmax_element(h->chan.begin(), h->chan.end());
            h->lo = *mm.first, h->hi = *mm.second;
        }
        h->bus_start_dev.upload(h->bus_start.data(), sizeof(int32_t) * h->bus_start.size());
        h->chan_dev.upload(h->chan.data(), sizeof(int32_t) * h->chan.size());
        h->gain_dev.upload(h->gain.data(), sizeof(float) * h->gain.size());
        *out = h.release();
    });
}

int rcfm_mix_run(rcfm_mix_t h, int first, int count, int A, int ch_in, const void* audio, const void* open, void* out, void* active,
                 void* bus_open, void* stream) {
    return guarded([&] {
        RC_REQUIRE(h && audio && out, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(ch_in == 1 || ch_in == 2, RCFM_ERR_ARG, "ch_in outside {1, 2}");
        RC_REQUIRE(count >= 1, RCFM_ERR_ARG, "count below 1");
        RC_REQUIRE(A >= 1, RCFM_ERR_ARG, "A below 1");
        const uintptr_t a0 = (uintptr_t)audio, o0 = (uintptr_t)out;
        RC_REQUIRE(a0 % 4 == 0 && o0 % 4 == 0 && (uintptr_t)active % 4 == 0, RCFM_ERR_ARG,
                   "misaligned buffer: audio and out are aligned for a float, active for an int32");
        const size_t row_in = (size_t)A * (size_t)ch_in, row_out = (size_t)A * (size_t)h->ch_out;
        const uintptr_t a1 = a0 + sizeof(float) * (size_t)count * row_in, o1 = o0 + sizeof(float) * (size_t)h->M * row_out;
        RC_REQUIRE(a1 <= o0 || o1 <= a0, RCFM_ERR_ARG, "out overlaps audio");
        RC_REQUIRE(h->hi < h->lo || ((int64_t)h->lo >= first && (int64_t)h->hi < (int64_t)first + count), RCFM_ERR_INDEX,
                   "a route's channel lies outside [first, first + count)");
        const bool vin = a0 % 16 == 0 && row_in % 4 == 0, vout = o0 % 16 == 0 && row_out % 4 == 0;
        const dim3 grid((unsigned)(((int64_t)A + kMixTile - 1) / kMixTile), (unsigned)h->M);
        auto go = [&](auto launch) {
            launch(vin, vout, grid, as_stream(stream), static_cast<const float*>(audio), static_cast<const uint8_t*>(open), first, A,
                   h->bus_start_dev.as<int32_t>(), h->chan_dev.as<int32_t>(), h->gain_dev.as<float2>(), static_cast<float*>(out),
                   static_cast<int32_t*>(active), static_cast<uint8_t*>(bus_open));
        };
        if (ch_in == 1 && h->ch_out == 1)
            go(launch_mix<1, 1>);
        else if (ch_in == 1)
            go(launch_mix<1, 2>);
        else if (h->ch_out == 1)
            go(launch_mix<2, 1>);
        else
            go(launch_mix<2, 2>);
    });
}

int rcfm_mix_destroy(rcfm_mix_t h) {
    return guarded([&] { delete h; });
}

}  // extern "C"
