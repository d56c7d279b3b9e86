// The wideband noise blanker (include/rcfm.h, "noise blanker"): rcfm_blanker_create, rcfm_blanker_run, rcfm_blanker_destroy,
// and rcfm_blanker_last of rcfm_tools.h.  An impulse is a few samples long only in the time-domain buffer, in front of the
// wideband FFT; the stage streams over that buffer: k_blank_level (float64 block sums), k_blank_fold (blocks longer than a
// tile), k_blank_threshold (the median of the neighbouring blocks), k_blank_hits (the hit bitmask) and k_blank_apply (the
// gain).  Detection is a pass of its own: an in-place run reads every sample a hit is decided from before any workgroup
// scales one.
//
// Every pass gives a workgroup one tile of kBlankTile samples and a lane V consecutive samples, 16 bytes, at a sample index
// that is a multiple of V.  Which lane holds which sample therefore follows from the sample's index alone; where the buffer
// is not 16-byte aligned, or at a tail, the same lane takes the same samples one by one.

#include <cmath>
#include <memory>
#include <vector>

#include "blanker.h"
#include "common.h"

namespace rcfm {

namespace {

template <int FORMAT>
struct BlankFormat;

template <>
struct BlankFormat<RCFM_IQ_CF32> {
    using Raw = uint2;                  // one sample's bits
    static constexpr int V = 2;         // samples in 16 bytes
    static __device__ __forceinline__ Raw none() { return make_uint2(0u, 0u); }
    static __device__ __forceinline__ void unpack(const uint4& v, Raw (&r)[V]) {
        r[0] = make_uint2(v.x, v.y);
        r[1] = make_uint2(v.z, v.w);
    }
    static __device__ __forceinline__ uint4 pack(const Raw (&r)[V]) { return make_uint4(r[0].x, r[0].y, r[1].x, r[1].y); }
    static __device__ __forceinline__ float2 value(Raw r) { return make_float2(__uint_as_float(r.x), __uint_as_float(r.y)); }
    static __device__ __forceinline__ Raw zero(int64_t) { return make_uint2(0u, 0u); }
    static __device__ __forceinline__ Raw scale(Raw r, float g) {
        return make_uint2(__float_as_uint(__fmul_rn(g, __uint_as_float(r.x))), __float_as_uint(__fmul_rn(g, __uint_as_float(r.y))));
    }
};

template <>
struct BlankFormat<RCFM_IQ_CS16> {
    using Raw = uint32_t;
    static constexpr int V = 4;
    static __device__ __forceinline__ Raw none() { return 0u; }
    static __device__ __forceinline__ void unpack(const uint4& v, Raw (&r)[V]) {
        r[0] = v.x;
        r[1] = v.y;
        r[2] = v.z;
        r[3] = v.w;
    }
    static __device__ __forceinline__ uint4 pack(const Raw (&r)[V]) { return make_uint4(r[0], r[1], r[2], r[3]); }
    static __device__ __forceinline__ int re(Raw r) { return (int16_t)(r & 0xffffu); }
    static __device__ __forceinline__ int im(Raw r) { return (int16_t)(r >> 16); }
    static __device__ __forceinline__ float2 value(Raw r) { return make_float2((float)re(r) * 0x1p-15f, (float)im(r) * 0x1p-15f); }
    static __device__ __forceinline__ Raw zero(int64_t) { return 0u; }
    static __device__ __forceinline__ Raw scale(Raw r, float g) {
        const int a = (int)rintf(__fmul_rn(g, (float)re(r))), b = (int)rintf(__fmul_rn(g, (float)im(r)));
        return ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16);
    }
};

// int8 and uint8 pairs: two bytes a sample, two samples a word
template <bool UNSIGNED>
struct BlankFormat8 {
    using Raw = uint16_t;
    static constexpr int V = 8;
    static __device__ __forceinline__ Raw none() { return UNSIGNED ? (Raw)0x7f7fu : (Raw)0u; }
    static __device__ __forceinline__ void unpack(const uint4& v, Raw (&r)[V]) {
        r[0] = (Raw)(v.x & 0xffffu);
        r[1] = (Raw)(v.x >> 16);
        r[2] = (Raw)(v.y & 0xffffu);
        r[3] = (Raw)(v.y >> 16);
        r[4] = (Raw)(v.z & 0xffffu);
        r[5] = (Raw)(v.z >> 16);
        r[6] = (Raw)(v.w & 0xffffu);
        r[7] = (Raw)(v.w >> 16);
    }
    static __device__ __forceinline__ uint4 pack(const Raw (&r)[V]) {
        return make_uint4((uint32_t)r[0] | ((uint32_t)r[1] << 16), (uint32_t)r[2] | ((uint32_t)r[3] << 16),
                          (uint32_t)r[4] | ((uint32_t)r[5] << 16), (uint32_t)r[6] | ((uint32_t)r[7] << 16));
    }
    // the integer as a float, the centre taken off: exact
    static __device__ __forceinline__ float code(unsigned byte) {
        return UNSIGNED ? (float)byte - 127.5f : (float)(int8_t)byte;
    }
    static __device__ __forceinline__ float2 value(Raw r) {
        return make_float2(code(r & 0xffu) * 0x1p-7f, code((unsigned)r >> 8) * 0x1p-7f);
    }
    static __device__ __forceinline__ Raw zero(int64_t i) {
        const unsigned c = UNSIGNED ? 127u + (unsigned)(i & 1) : 0u;     // 127.5 is not a code: 127, 128, 127, ...
        return (Raw)(c | (c << 8));
    }
    static __device__ __forceinline__ unsigned scaled(unsigned byte, float g) {
        const float y = __fmul_rn(g, code(byte));
        return (unsigned)(int)rintf(UNSIGNED ? __fadd_rn(127.5f, y) : y) & 0xffu;
    }
    static __device__ __forceinline__ Raw scale(Raw r, float g) {
        return (Raw)(scaled(r & 0xffu, g) | (scaled((unsigned)r >> 8, g) << 8));
    }
};
template <>
struct BlankFormat<RCFM_IQ_CS8> : BlankFormat8<false> {};
template <>
struct BlankFormat<RCFM_IQ_CU8> : BlankFormat8<true> {};

// The V samples from index i0 (a multiple of V, below n) on: one 16-byte load where the buffer allows it, sample by sample
// otherwise; slots at and beyond n hold none().
template <int FORMAT>
__device__ __forceinline__ void blank_load(const void* __restrict__ in, int64_t i0, int64_t n, bool vec,
                                           typename BlankFormat<FORMAT>::Raw (&r)[BlankFormat<FORMAT>::V]) {
    using F = BlankFormat<FORMAT>;
    using Raw = typename F::Raw;
    const Raw* x = static_cast<const Raw*>(in);
    if (vec && i0 + F::V <= n) {
        F::unpack(*reinterpret_cast<const uint4*>(x + i0), r);
    } else {
#pragma unroll
        for (int k = 0; k < F::V; ++k) r[k] = i0 + k < n ? x[i0 + k] : F::none();
    }
}

// First sample of the V a lane takes in sweep `it` of its wave's run, counted from the tile's first sample.
template <int V>
__device__ __forceinline__ int blank_offset(int it) {
    return (int)(threadIdx.x >> 6) * kBlankWaveRun + it * 64 * V + (int)(threadIdx.x & 63) * V;
}

__device__ __forceinline__ void blank_count(int v, unsigned long long* slot) {
    __shared__ int wave_count[kBlankThreads / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int tot = 0;
    for (int w = 0; w < kBlankThreads / 64; ++w) tot += wave_count[w];
    if (tot) atomicAdd(slot, (unsigned long long)tot);
}

// Block sums in float64: sums[b] = the pairwise tree over block b's L slots, slots at and beyond n being zero -- node j of a
// level is node 2 j + node 2 j + 1 of the level below, whatever the format, the alignment or the grid.  A lane adds its V
// samples as that tree's lowest levels, the wave's xor shuffles are the next ones up to `seg` = min(L, 64 V) samples, and
// one thread per output folds the tile's `seg` sums in LDS up to min(L, kBlankTile).  L <= kBlankTile: sums is [nb];
// longer blocks: [tiles], for k_blank_fold.  The first thread of the launch zeroes stats on the way.
template <int FORMAT>
__global__ __launch_bounds__(kBlankThreads) void k_blank_level(const void* __restrict__ in, int64_t n, int log2l, bool vec,
                                                               double* __restrict__ sums, unsigned long long* __restrict__ stats) {
    using F = BlankFormat<FORMAT>;
    constexpr int V = F::V, kSweeps = kBlankWaveRun / (64 * V);
    __shared__ double ent[kBlankTile / kBlankMinBlock];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t tile0 = (int64_t)blockIdx.x * kBlankTile;
    const int seg = min(1 << min(log2l, 12), 64 * V);
    const int lanes = seg / V;
    if (stats != nullptr && blockIdx.x == 0 && tid == 0) stats[0] = stats[1] = 0;     // the later passes count into them
#pragma unroll
    for (int it = 0; it < kSweeps; ++it) {
        const int off = blank_offset<V>(it);
        const int64_t i0 = tile0 + off;
        double s[V];
        if (i0 < n) {                               // (wave-uniform or not: the shuffles below are outside)
            typename F::Raw r[V];
            blank_load<FORMAT>(in, i0, n, vec, r);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float2 x = F::value(r[k]);
                const double re = x.x, im = x.y;
                s[k] = i0 + k < n ? re * re + im * im : 0.0;     // both products are exact: one rounding, contracted or not
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = 0.0;
        }
#pragma unroll
        for (int w = 1; w < V; w <<= 1)
#pragma unroll
            for (int k = 0; k < V; k += 2 * w) s[k] += s[k + w];
        double v = s[0];
        for (int d = 1; d < lanes; d <<= 1) v += __shfl_xor(v, d, 64);
        if ((lane & (lanes - 1)) == 0) ent[off / seg] = v;
    }
    __syncthreads();
    const int per = (1 << min(log2l, 12)) / seg;        // entries of one output
    const int outputs = kBlankTile / seg / per;
    if (tid >= outputs) return;
    double* e = ent + tid * per;
    for (int w = 1; w < per; w <<= 1)
        for (int k = 0; k < per; k += 2 * w) e[k] += e[k + w];
    if (log2l >= 12) {
        sums[blockIdx.x] = e[0];
    } else {
        const int64_t first = tile0 + ((int64_t)tid << log2l);
        if (first < n) sums[first >> log2l] = e[0];
    }
}

// Blocks of k = L / kBlankTile tiles, 2 <= k <= 256: workgroup b continues the tree over its tiles' sums.
__global__ __launch_bounds__(kBlankThreads) void k_blank_fold(const double* __restrict__ part, int64_t tiles, int k,
                                                              double* __restrict__ sums) {
    __shared__ double wave_sum[kBlankThreads / 64];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * k + tid;
    double v = tid < k && c < tiles ? part[c] : 0.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// One thread per block: m = sum / count (a non-finite one counts as +inf), the lower median r of m over the blocks within W,
// t = (float)(value r).  The workgroup stages its blocks' means and W more each side in LDS; a thread then finds the element
// of rank (cnt - 1) / 2 by counting, ties in index order -- the element an ascending stable sort puts there.
__global__ __launch_bounds__(kBlankThreads) void k_blank_threshold(const double* __restrict__ sums, int64_t nb, int64_t n,
                                                                   int log2l, int W, double value, float* __restrict__ t) {
#pragma clang fp contract(off)
    __shared__ double win[kBlankThreads + 2 * kBlankMaxSpan];
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kBlankThreads;
    for (int j = tid; j < kBlankThreads + 2 * W; j += kBlankThreads) {
        const int64_t b = b0 - W + j;
        double m = __builtin_inf();
        if (b >= 0 && b < nb) {
            const int64_t first = b << log2l;
            const int64_t cnt = n - first < ((int64_t)1 << log2l) ? n - first : (int64_t)1 << log2l;
            m = sums[b] / (double)cnt;
            if (!isfinite(m)) m = __builtin_inf();
        }
        win[j] = m;
    }
    __syncthreads();
    const int64_t b = b0 + tid;
    if (b >= nb) return;
    const int lo = (int)(b - W < 0 ? -b : -W), hi = (int)(b + W > nb - 1 ? nb - 1 - b : W);     // relative to b
    const int want = (hi - lo) / 2;                                                              // (cnt - 1) / 2
    double r = 0.0;
    for (int i = lo; i <= hi; ++i) {
        const double vi = win[tid + W + i];
        int rank = 0;
        for (int j = lo; j <= hi; ++j) {
            const double vj = win[tid + W + j];
            rank += (vj < vi || (vj == vi && j < i)) ? 1 : 0;
        }
        if (rank == want) r = vi;
    }
    t[b] = (float)(value * r);
}

// hit[i] = p[i] > t[block of i], p = fl32(fl32(re re) + fl32(im im)): the tile's 128 mask words, whole, bits at and beyond n
// zero.  A lane's V hit bits, shifted to their place, are ORed over the 32 / V lanes of a word.  stats[0] += the tile's hits.
template <int FORMAT>
__global__ __launch_bounds__(kBlankThreads) void k_blank_hits(const void* __restrict__ in, int64_t n, int log2l, bool vec,
                                                              const float* __restrict__ t, uint32_t* __restrict__ mask,
                                                              unsigned long long* __restrict__ stats) {
    using F = BlankFormat<FORMAT>;
    constexpr int V = F::V, kSweeps = kBlankWaveRun / (64 * V), kWordLanes = 32 / V;
    const int lane = threadIdx.x & 63;
    const int64_t tile0 = (int64_t)blockIdx.x * kBlankTile;
    int count = 0;
#pragma unroll
    for (int it = 0; it < kSweeps; ++it) {
        const int off = blank_offset<V>(it);
        const int64_t i0 = tile0 + off;
        uint32_t bits = 0;
        if (i0 < n) {
            typename F::Raw r[V];
            blank_load<FORMAT>(in, i0, n, vec, r);
            const float tb = t[i0 >> log2l];            // V divides L: the lane's samples share a block
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float2 x = F::value(r[k]);
                const float p = __fadd_rn(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y));
                if (i0 + k < n && p > tb) bits |= 1u << k;
            }
        }
        count += __popc(bits);
        uint32_t word = bits << ((lane & (kWordLanes - 1)) * V);
#pragma unroll
        for (int d = 1; d < kWordLanes; d <<= 1) word |= __shfl_xor(word, d, 64);
        if ((lane & (kWordLanes - 1)) == 0) mask[(tile0 + off) >> 5] = word;
    }
    if (stats != nullptr) blank_count(count, stats);
}

// Distance from window bit q to the nearest set bit at or above it (UP) or at or below it, looking `scan` words beyond q's
// own; `far` when there is none.  win: the tile's mask words with kBlankHaloWords more each side, so q's word is at least
// kBlankHaloWords from either end and scan <= kBlankHaloWords stays inside.
template <bool UP>
__device__ __forceinline__ int blank_nearest(const uint32_t* win, int q, int scan, int far) {
    int wi = q >> 5;
    const int bi = q & 31;
    uint32_t w = win[wi] & (UP ? ~0u << bi : ~0u >> (31 - bi));
    for (int s = 0;; ++s) {
        if (w != 0) return UP ? (wi << 5) + (__ffs(w) - 1) - q : q - ((wi << 5) + 31 - __clz(w));
        if (s == scan) return far;
        wi += UP ? 1 : -1;
        w = win[wi];
    }
}

// One tile: out = g in, g from the distance to the nearest hit.  The workgroup reads the mask words of the tile and of G
// samples each side.  No hit among them: nothing to do in place, a 16-byte copy otherwise.  With a hit every sample finds its
// distance by scanning words -- after a look at the few words around its own V samples, which are zero for most lanes even
// of such a tile; in place only the samples with g < 1 are stored.  stats[1] += the tile's samples with g < 1.
template <int FORMAT>
__global__ __launch_bounds__(kBlankThreads) void k_blank_apply(const void* in, void* out, int64_t n, bool vec,
                                                               const uint32_t* __restrict__ mask, int64_t nwords, int H, int G,
                                                               const float* __restrict__ ramp,
                                                               unsigned long long* __restrict__ stats) {
    using F = BlankFormat<FORMAT>;
    using Raw = typename F::Raw;
    constexpr int V = F::V, kSweeps = kBlankWaveRun / (64 * V);
    __shared__ uint32_t win[kBlankWindowWords];
    __shared__ float gain[kBlankMaxGuard];
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * kBlankTile;
    const int scan = (G + 31) / 32;
    bool near = false;
    if (tid < kBlankWindowWords) {
        const int64_t idx = (int64_t)blockIdx.x * kBlankTileWords - kBlankHaloWords + tid;
        const uint32_t w = idx >= 0 && idx < nwords ? mask[idx] : 0u;
        win[tid] = w;
        near = w != 0 && tid >= kBlankHaloWords - scan && tid < kBlankHaloWords + kBlankTileWords + scan;
    }
    const bool in_place = in == out;
    Raw* y = static_cast<Raw*>(out);
    if (!__syncthreads_or(near)) {
        if (in_place) return;
#pragma unroll
        for (int it = 0; it < kSweeps; ++it) {
            const int64_t i0 = tile0 + blank_offset<V>(it);
            if (i0 >= n) continue;
            Raw r[V];
            blank_load<FORMAT>(in, i0, n, vec, r);
            if (vec && i0 + V <= n) {
                *reinterpret_cast<uint4*>(y + i0) = F::pack(r);
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (i0 + k < n) y[i0 + k] = r[k];
            }
        }
        return;
    }
    for (int j = tid; j < G - H; j += kBlankThreads) gain[j] = ramp[j];
    __syncthreads();
    int blanked = 0;
#pragma unroll
    for (int it = 0; it < kSweeps; ++it) {
        const int off = blank_offset<V>(it);
        const int64_t i0 = tile0 + off;
        if (i0 >= n) continue;
        // the words that hold the bits within G of the lane's samples: all zero for most lanes of most such tiles
        const int q0 = kBlankMaxGuard + off;
        uint32_t any = 0;
        for (int w = (q0 - G) >> 5; w <= (q0 + V - 1 + G) >> 5; ++w) any |= win[w];
        if (any == 0 && in_place) continue;
        Raw r[V];
        blank_load<FORMAT>(in, i0, n, vec, r);
        bool keep[V];
#pragma unroll
        for (int k = 0; k < V; ++k) keep[k] = true;
        if (any != 0) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int q = q0 + k;
                const int d = min(blank_nearest<true>(win, q, scan, G + 1), blank_nearest<false>(win, q, scan, G + 1));
                const float g = d <= H ? 0.f : d <= G ? gain[d - H - 1] : 1.f;
                keep[k] = g == 1.f || i0 + k >= n;
                if (!keep[k]) {
                    r[k] = g == 0.f ? F::zero(i0 + k) : F::scale(r[k], g);
                    ++blanked;
                }
            }
        }
        if (!in_place && vec && i0 + V <= n) {
            *reinterpret_cast<uint4*>(y + i0) = F::pack(r);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (i0 + k < n && !(in_place && keep[k])) y[i0 + k] = r[k];
        }
    }
    if (stats != nullptr) blank_count(blanked, stats + 1);
}

size_t blank_sample_bytes(int format) { return format == RCFM_IQ_CF32 ? 8 : format == RCFM_IQ_CS16 ? 4 : 2; }

}  // namespace

}  // namespace rcfm

using namespace rcfm;

struct rcfm_blanker {
    int64_t n_max = 0;
    int log2l = 0, W = 0, mode = 0, H = 0, G = 0;
    double value = 0.0;
    DeviceBuffer sums, part, t, mask, ramp;     // float64 [nb], float64 [tiles] (blocks longer than a tile), float32 [nb],
                                                // uint32 [tiles][kBlankTileWords], float32 [G - H]
    int64_t last_nb = 0;
};

namespace rcfm {

namespace {

template <int FORMAT>
void blank_launch(rcfm_blanker& b, int64_t n, const void* in, void* out, unsigned long long* stats, hipStream_t s) {
    const int64_t tiles = blank_tiles(n), nb = (n + ((int64_t)1 << b.log2l) - 1) >> b.log2l;
    const dim3 grid((unsigned)tiles), block(kBlankThreads);
    const bool vec_in = (uintptr_t)in % 16 == 0, vec_both = vec_in && (uintptr_t)out % 16 == 0;
    if (b.mode == RCFM_BLANK_MEDIAN) {
        const bool longer = b.log2l > 12;
        hipLaunchKernelGGL(k_blank_level<FORMAT>, grid, block, 0, s, in, n, b.log2l, vec_in,
                           longer ? b.part.as<double>() : b.sums.as<double>(), stats);
        RC_HIP(hipGetLastError());
        if (longer) {
            hipLaunchKernelGGL(k_blank_fold, dim3((unsigned)nb), block, 0, s, b.part.as<double>(), tiles, 1 << (b.log2l - 12),
                               b.sums.as<double>());
            RC_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k_blank_threshold, dim3((unsigned)((nb + kBlankThreads - 1) / kBlankThreads)), block, 0, s,
                           b.sums.as<double>(), nb, n, b.log2l, b.W, b.value, b.t.as<float>());
        RC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_blank_hits<FORMAT>, grid, block, 0, s, in, n, b.log2l, vec_in, b.t.as<float>(), b.mask.as<uint32_t>(),
                       stats);
    RC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_blank_apply<FORMAT>, grid, block, 0, s, in, out, n, vec_both, b.mask.as<uint32_t>(),
                       tiles * kBlankTileWords, b.H, b.G, b.ramp.as<float>(), stats);
    RC_HIP(hipGetLastError());
    b.last_nb = nb;
}

}  // namespace

}  // namespace rcfm

extern "C" {

int rcfm_blanker_create(int64_t n_max, int block, int span, int mode, double value, int hold, const float* ramp_host, int ramp,
                        rcfm_blanker_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(n_max >= 1 && n_max <= kBlankMaxSamples, RCFM_ERR_ARG, "n_max outside 1 .. 2^40");
        RC_REQUIRE(block >= kBlankMinBlock && block <= (1 << kBlankMaxBlockLog2) && (block & (block - 1)) == 0, RCFM_ERR_ARG,
                   "the block length is a power of two, 64 .. 2^20");
        RC_REQUIRE(span >= 0 && span <= kBlankMaxSpan, RCFM_ERR_ARG, "the half-span is 0 .. 8 blocks");
        RC_REQUIRE(mode == RCFM_BLANK_MEDIAN || mode == RCFM_BLANK_ABSOLUTE, RCFM_ERR_ARG,
                   "unknown blanker mode (RCFM_BLANK_MEDIAN, RCFM_BLANK_ABSOLUTE)");
        RC_REQUIRE(std::isfinite(value) && value > 0.0, RCFM_ERR_ARG, "the threshold value must be finite and positive");
        RC_REQUIRE(hold >= 0 && hold <= kBlankMaxGuard && ramp >= 0 && ramp <= kBlankMaxGuard && hold + ramp <= kBlankMaxGuard,
                   RCFM_ERR_ARG, "hold and ramp are not negative and hold + ramp is at most 1024 samples");
        RC_REQUIRE(ramp == 0 || ramp_host != nullptr, RCFM_ERR_ARG, "NULL ramp table");
        for (int j = 0; j < ramp; ++j)
            RC_REQUIRE(std::isfinite(ramp_host[j]) && ramp_host[j] >= 0.f && ramp_host[j] <= 1.f, RCFM_ERR_ARG,
                       "a ramp value is not finite or outside 0 .. 1");
        auto b = std::make_unique<rcfm_blanker>();
        b->n_max = n_max;
        while ((1 << b->log2l) < block) ++b->log2l;
        b->W = span;
        b->mode = mode;
        b->value = value;
        b->H = hold;
        b->G = hold + ramp;
        const int64_t tiles = blank_tiles(n_max), nb = (n_max + block - 1) / block;
        b->mask.reset((size_t)tiles * kBlankTileWords * sizeof(uint32_t));
        if (mode == RCFM_BLANK_MEDIAN) {
            b->sums.reset((size_t)nb * sizeof(double));
            if (block > kBlankTile) b->part.reset((size_t)tiles * sizeof(double));
            b->t.reset((size_t)nb * sizeof(float));
        } else {
            const std::vector<float> t((size_t)nb, (float)value);
            b->t.upload(t.data(), t.size() * sizeof(float));
        }
        if (ramp > 0) b->ramp.upload(ramp_host, (size_t)ramp * sizeof(float));
        *out = b.release();
    });
}

int rcfm_blanker_run(rcfm_blanker_t b, int format, int64_t n, const void* in, void* out, void* stats, void* stream) {
    return guarded([&] {
        RC_REQUIRE(b != nullptr, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(format == RCFM_IQ_CF32 || format == RCFM_IQ_CS16 || format == RCFM_IQ_CS8 || format == RCFM_IQ_CU8, RCFM_ERR_ARG,
                   "unknown sample format (RCFM_IQ_CF32, RCFM_IQ_CS16, RCFM_IQ_CS8, RCFM_IQ_CU8)");
        RC_REQUIRE(n >= 0 && n <= b->n_max, RCFM_ERR_ARG, "n outside 0 .. n_max of the handle");
        RC_REQUIRE((uintptr_t)stats % 8 == 0, RCFM_ERR_ARG, "misaligned buffer: stats is aligned for an int64");
        hipStream_t s = as_stream(stream);
        if (n > 0) {
            RC_REQUIRE(in != nullptr && out != nullptr, RCFM_ERR_ARG, "NULL buffer");
            const size_t elem = blank_sample_bytes(format);
            RC_REQUIRE((uintptr_t)in % elem == 0 && (uintptr_t)out % elem == 0, RCFM_ERR_ARG,
                       "misaligned buffer: in and out are aligned for one sample of the format");
            const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out, bytes = (uintptr_t)n * elem;
            RC_REQUIRE(a == o || a + bytes <= o || o + bytes <= a, RCFM_ERR_ARG,
                       "in and out overlap in part: they are the same buffer or disjoint");
        }
        // (a median run's level pass zeroes stats itself)
        if (stats != nullptr && (n == 0 || b->mode == RCFM_BLANK_ABSOLUTE)) RC_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), s));
        if (n == 0) {
            b->last_nb = 0;
            return;
        }
        unsigned long long* st = static_cast<unsigned long long*>(stats);
        switch (format) {
            case RCFM_IQ_CF32: blank_launch<RCFM_IQ_CF32>(*b, n, in, out, st, s); break;
            case RCFM_IQ_CS16: blank_launch<RCFM_IQ_CS16>(*b, n, in, out, st, s); break;
            case RCFM_IQ_CS8: blank_launch<RCFM_IQ_CS8>(*b, n, in, out, st, s); break;
            default: blank_launch<RCFM_IQ_CU8>(*b, n, in, out, st, s); break;
        }
    });
}

int rcfm_blanker_destroy(rcfm_blanker_t b) {
    return guarded([&] { delete b; });
}

int rcfm_blanker_last(rcfm_blanker_t b, void** t_dev, void** hit_words_dev, int64_t* nb) {
    return guarded([&] {
        RC_REQUIRE(b != nullptr, RCFM_ERR_ARG, "NULL handle");
        if (t_dev != nullptr) *t_dev = b->t.get();
        if (hit_words_dev != nullptr) *hit_words_dev = b->mask.get();
        if (nb != nullptr) *nb = b->last_nb;
    });
}

}  // extern "C"
