// Per-row power-of-two scaling of AM / SSB channels that share a complex transform (pair_scale.h).

#include "pair_scale.h"

#include "common.h"

namespace rcfm {

namespace {

constexpr int kWaves = kPairScaleThreads / 64;

// The largest of the workgroup's m, in every thread.  fmaxf drops a NaN, so a row with NaNs is scaled by its finite
// samples and keeps its NaNs.
__device__ __forceinline__ float block_max(float m, float* red) {
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    float top = red[0];
    for (int w = 1; w < kWaves; ++w) top = fmaxf(top, red[w]);
    return top;
}

// e with m 2^e in [1, 2), kept to the exponents whose power and inverse power are both normal; 0 for a row that is
// silent or not finite.
__device__ __forceinline__ int pair_exponent(float m) {
    if (!(m > 0.f) || !(m <= 3.402823466e38f)) return 0;
    const int e = -ilogbf(m);
    return e < -126 ? -126 : (e > 126 ? 126 : e);
}

__device__ __forceinline__ void store_factors(float* scale, int rows, int r, int e) {
    scale[r] = ldexpf(1.f, e);
    scale[rows + r] = ldexpf(1.f, -e);
}

// Row blockIdx.x of e [rows][n]: its largest magnitude, then the row times 2^e in place (the second sweep re-reads what
// the first left in cache).  VEC (n % 4 == 0 and e 16-byte aligned): 16-byte accesses.
template <bool VEC>
__global__ __launch_bounds__(kPairScaleThreads) void k_am_pair_scale(float* __restrict__ e, int64_t n, int rows,
                                                                     float* __restrict__ scale) {
    __shared__ float red[kWaves];
    const int tid = threadIdx.x, r = blockIdx.x;
    float* row = e + (int64_t)r * n;
    float m = 0.f;
    if (VEC) {
        for (int64_t i = 4 * (int64_t)tid; i < n; i += 4 * kPairScaleThreads) {
            const float4 v = *reinterpret_cast<const float4*>(row + i);
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    } else {
        for (int64_t i = tid; i < n; i += kPairScaleThreads) m = fmaxf(m, fabsf(row[i]));
    }
    const int ex = pair_exponent(block_max(m, red));
    if (tid == 0) store_factors(scale, rows, r, ex);
    if (ex == 0) return;
    const float f = ldexpf(1.f, ex);
    if (VEC) {
        for (int64_t i = 4 * (int64_t)tid; i < n; i += 4 * kPairScaleThreads) {
            const float4 v = *reinterpret_cast<const float4*>(row + i);
            *reinterpret_cast<float4*>(row + i) = make_float4(v.x * f, v.y * f, v.z * f, v.w * f);
        }
    } else {
        for (int64_t i = tid; i < n; i += kPairScaleThreads) row[i] *= f;
    }
}

// Channel blockIdx.x: the largest |re|, |im| over the sideband bins 1 .. kmax, addressed as LoadSsbPairT::bin does.
__global__ __launch_bounds__(kPairScaleThreads) void k_ssb_pair_scale(const float2* __restrict__ X,
                                                                      const int32_t* __restrict__ base32, int B, int kmax,
                                                                      int lower, int rows, float* __restrict__ scale) {
    __shared__ float red[kWaves];
    const int tid = threadIdx.x, c = blockIdx.x;
    const float2* Xc = base32 ? X + base32[c] : X + (int64_t)c * B;
    float m = 0.f;
    for (int kk = 1 + tid; kk <= kmax; kk += kPairScaleThreads) {
        const int q = lower ? -kk : kk;
        const float2 v = Xc[(!base32 && q < 0) ? B + q : q];
        m = fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y)));
    }
    const int ex = pair_exponent(block_max(m, red));
    if (tid == 0) store_factors(scale, rows, c, ex);
}

template <bool VEC>
__global__ __launch_bounds__(kPairScaleThreads) void k_rows_rescale(float* __restrict__ y, int64_t n,
                                                                    const float* __restrict__ factor) {
    const int tid = threadIdx.x;
    float* row = y + (int64_t)blockIdx.x * n;
    const float f = factor[blockIdx.x];
    if (f == 1.f) return;
    if (VEC) {
        for (int64_t i = 4 * (int64_t)tid; i < n; i += 4 * kPairScaleThreads) {
            const float4 v = *reinterpret_cast<const float4*>(row + i);
            *reinterpret_cast<float4*>(row + i) = make_float4(v.x * f, v.y * f, v.z * f, v.w * f);
        }
    } else {
        for (int64_t i = tid; i < n; i += kPairScaleThreads) row[i] *= f;
    }
}

bool vec_rows(const float* p, int64_t n) { return n % 4 == 0 && ((uintptr_t)p & 15) == 0; }

}  // namespace

void launch_am_pair_scale(float* e, int64_t n, int rows, float* scale, hipStream_t stream) {
    if (rows <= 0 || n <= 0) return;
    const dim3 grid((unsigned)rows), block(kPairScaleThreads);
    if (vec_rows(e, n))
        hipLaunchKernelGGL(k_am_pair_scale<true>, grid, block, 0, stream, e, n, rows, scale);
    else
        hipLaunchKernelGGL(k_am_pair_scale<false>, grid, block, 0, stream, e, n, rows, scale);
    RC_HIP(hipGetLastError());
}

void launch_ssb_pair_scale(const float2* X, const int32_t* base32, int B, int kmax, bool lower, int rows, float* scale,
                           hipStream_t stream) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_ssb_pair_scale, dim3((unsigned)rows), dim3(kPairScaleThreads), 0, stream, X, base32, B, kmax,
                       lower ? 1 : 0, rows, scale);
    RC_HIP(hipGetLastError());
}

void launch_rows_rescale(float* y, int64_t n, int rows, const float* factor, hipStream_t stream) {
    if (rows <= 0 || n <= 0) return;
    const dim3 grid((unsigned)rows), block(kPairScaleThreads);
    if (vec_rows(y, n))
        hipLaunchKernelGGL(k_rows_rescale<true>, grid, block, 0, stream, y, n, factor);
    else
        hipLaunchKernelGGL(k_rows_rescale<false>, grid, block, 0, stream, y, n, factor);
    RC_HIP(hipGetLastError());
}

}  // namespace rcfm
