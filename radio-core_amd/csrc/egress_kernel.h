// Kernels of the audio egress (rcfm_audio_pack, include/rcfm.h): the slot scan and the pack.  A header of its own so that
// tools/microbench/pack_store_ab.hip times the very kernel the library launches, with either store form.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rcfm.h"

namespace rcfm {

constexpr int kScanThreads = 1024;   // ONE workgroup scans the whole mask: 65 535 bytes are at most 64 per thread
constexpr int kPackThreads = 256;
// Elements of a row per workgroup and sweep: RCFM_PACK_SEGMENT of radiocore/_internal/hip.py (the tests put a row on each
// side of it).  Per lane that is two 16-byte stores of eight int16 (four 16-byte loads), or four float4 in and out.
constexpr int kPackSegment = 16 * kPackThreads;

// slot[c] = the number of open channels below c for an open channel c (open == nullptr: every channel), -1 for a closed one;
// index[slot[c]] = c; *n_open = the number of open channels.  index and n_open may be null.  Thread t owns channels
// [t per, (t + 1) per), per = ceil(count / kScanThreads): it counts its open ones, the counts are scanned across the
// workgroup in LDS (integers: one result whatever the order), and a second sweep over the same channels hands out the slots.
__global__ __launch_bounds__(kScanThreads) void k_slot_scan(const uint8_t* __restrict__ open, int count, int32_t* __restrict__ slot,
                                                            int32_t* __restrict__ index, int32_t* __restrict__ n_open) {
    __shared__ int part[kScanThreads];
    const int tid = threadIdx.x;
    const int per = (count + kScanThreads - 1) / kScanThreads;
    const int lo = min(tid * per, count), hi = min(lo + per, count);
    int n = 0;
    for (int c = lo; c < hi; ++c) n += (open == nullptr || open[c] != 0) ? 1 : 0;
    part[tid] = n;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int s = part[tid] - n;
    for (int c = lo; c < hi; ++c) {
        const bool is_open = open == nullptr || open[c] != 0;
        slot[c] = is_open ? s : -1;
        if (is_open) {
            if (index != nullptr) index[s] = c;
            ++s;
        }
    }
    if (tid == kScanThreads - 1 && n_open != nullptr) *n_open = part[tid];
}

// RCFM_PCM_S16 of one sample: one float32 multiply, NaN -> 0, round to nearest even, clamp to +-32767.  The clamp comes
// first: its bounds are integers and the rounding is monotone, so the result is the same, and +-inf never reach the convert.
__device__ __forceinline__ int pcm_s16(float x, float gain) {
    const float y = x * gain;
    const float r = rintf(fminf(fmaxf(y, -32767.0f), 32767.0f));
    return y != y ? 0 : (int)r;
}

__device__ __forceinline__ unsigned pcm_s16_pair(float lo, float hi, float gain) {
    return ((unsigned)pcm_s16(lo, gain) & 0xffffu) | ((unsigned)pcm_s16(hi, gain) << 16);
}

typedef unsigned int pack_u4 __attribute__((ext_vector_type(4)));

template <bool NT, class T>
__device__ __forceinline__ void pack_store(T v, T* p) {
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// Channel blockIdx.x, when open, to row slot[blockIdx.x] of `packed`; segments blockIdx.y, blockIdx.y + gridDim.y, ... of
// kPackSegment elements each.  A closed channel's workgroups leave before they read a byte of its row.
// VEC (both bases 16-byte aligned; row % 8 == 0 for S16, row % 4 == 0 for F32: every row starts aligned on both sides):
//   S16  a lane loads two float4 and stores eight int16 as one 16-byte vector, twice per segment;
//   F32  a lane moves four 16-byte vectors per segment, as 32-bit integers: the bits of a NaN pass unchanged.
// Otherwise one element per lane, 16 per segment.  All loads of a segment are issued before its first store.
// NT: non-temporal stores (nothing on the device reads `packed` back; the next reader is the copy engine).  Measured
// slower with every channel open, so the library launches NT = false (docs/EXPERIMENTS.md, "pack stores").
template <int FORMAT, bool VEC, bool NT>
__global__ __launch_bounds__(kPackThreads) void k_audio_pack(const float* __restrict__ audio, const int32_t* __restrict__ slot,
                                                             size_t row, float gain, void* __restrict__ packed) {
    const int s = slot[blockIdx.x];
    if (s < 0) return;
    const int tid = threadIdx.x;
    const float* a = audio + (size_t)blockIdx.x * row;
    for (size_t s0 = (size_t)blockIdx.y * kPackSegment; s0 < row; s0 += (size_t)gridDim.y * kPackSegment) {
        if (FORMAT == RCFM_PCM_S16) {
            int16_t* p = static_cast<int16_t*>(packed) + (size_t)s * row;
            if (VEC) {
                float4 v[2][2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const size_t i = s0 + 8 * (size_t)(j * kPackThreads + tid);
                    if (i < row) {
                        v[j][0] = *reinterpret_cast<const float4*>(a + i);
                        v[j][1] = *reinterpret_cast<const float4*>(a + i + 4);
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const size_t i = s0 + 8 * (size_t)(j * kPackThreads + tid);
                    if (i < row) {
                        pack_u4 o;
                        o.x = pcm_s16_pair(v[j][0].x, v[j][0].y, gain);
                        o.y = pcm_s16_pair(v[j][0].z, v[j][0].w, gain);
                        o.z = pcm_s16_pair(v[j][1].x, v[j][1].y, gain);
                        o.w = pcm_s16_pair(v[j][1].z, v[j][1].w, gain);
                        pack_store<NT>(o, reinterpret_cast<pack_u4*>(p + i));
                    }
                }
            } else {
                float v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const size_t i = s0 + (size_t)(j * kPackThreads + tid);
                    if (i < row) v[j] = a[i];
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const size_t i = s0 + (size_t)(j * kPackThreads + tid);
                    if (i < row) pack_store<NT>((int16_t)pcm_s16(v[j], gain), p + i);
                }
            }
        } else {
            uint32_t* p = static_cast<uint32_t*>(packed) + (size_t)s * row;
            const uint32_t* b = reinterpret_cast<const uint32_t*>(a);
            if (VEC) {
                pack_u4 v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t i = s0 + 4 * (size_t)(j * kPackThreads + tid);
                    if (i < row) v[j] = *reinterpret_cast<const pack_u4*>(b + i);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t i = s0 + 4 * (size_t)(j * kPackThreads + tid);
                    if (i < row) pack_store<NT>(v[j], reinterpret_cast<pack_u4*>(p + i));
                }
            } else {
                uint32_t v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const size_t i = s0 + (size_t)(j * kPackThreads + tid);
                    if (i < row) v[j] = b[i];
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const size_t i = s0 + (size_t)(j * kPackThreads + tid);
                    if (i < row) pack_store<NT>(v[j], p + i);
                }
            }
        }
    }
}

}  // namespace rcfm
