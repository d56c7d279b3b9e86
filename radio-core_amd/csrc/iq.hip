// Raw integer IQ -> complex64 (include/rcfm.h, RCFM_IQ_*): the stand-alone conversion behind rcfm_iq_convert, and what
// rcfm_tuner_load_raw runs in front of the complex64 load where the wideband FFT does not run on the engine.  (On the
// engine the same arithmetic rides on the first pass's load: fft_kernel.h, LoadIq16 / LoadIq8 / LoadIqU8.)

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace rcfm {

namespace {

constexpr int kIqThreads = 256;
constexpr size_t kIqMaxBlocks = 1 << 16;   // (grid-stride beyond: 2^25 samples per sweep)

template <int FORMAT>
struct IqFormat;
template <>
struct IqFormat<RCFM_IQ_CS16> {
    using T = int16_t;
    static __device__ __forceinline__ float value(T v) { return (float)v * 0x1p-15f; }
};
template <>
struct IqFormat<RCFM_IQ_CS8> {
    using T = int8_t;
    static __device__ __forceinline__ float value(T v) { return (float)v * 0x1p-7f; }
};
template <>
struct IqFormat<RCFM_IQ_CU8> {
    using T = uint8_t;
    static __device__ __forceinline__ float value(T v) { return ((float)v - 127.5f) * 0x1p-7f; }
};

// out[e] = (value(in[2 e]), value(in[2 e + 1])), e in [0, n).  `in` is aligned for one integer only, so every integer is
// a load of its own; the output is 8-byte aligned, and `head` (0 or 1) elements in front make the rest 16-byte aligned:
// lane j of the sweep stores elements head + 2 j and head + 2 j + 1 as one float4, and the first thread of the launch takes
// the head and, where n - head is odd, the last element.
template <int FORMAT>
__global__ __launch_bounds__(kIqThreads) void k_iq_convert(const typename IqFormat<FORMAT>::T* __restrict__ in,
                                                           float2* __restrict__ out, size_t n, unsigned head) {
    using F = IqFormat<FORMAT>;
    const size_t gid = (size_t)blockIdx.x * kIqThreads + threadIdx.x, stride = (size_t)gridDim.x * kIqThreads;
    const size_t pairs = (n - head) / 2;
    for (size_t j = gid; j < pairs; j += stride) {
        const size_t e = head + 2 * j;
        const float4 v = make_float4(F::value(in[2 * e]), F::value(in[2 * e + 1]), F::value(in[2 * e + 2]),
                                     F::value(in[2 * e + 3]));
        *reinterpret_cast<float4*>(out + e) = v;
    }
    if (gid == 0) {
        if (head) out[0] = make_float2(F::value(in[0]), F::value(in[1]));
        const size_t e = head + 2 * pairs;
        if (e < n) out[e] = make_float2(F::value(in[2 * e]), F::value(in[2 * e + 1]));
    }
}

template <int FORMAT>
void launch_one(size_t n, const void* in, float2* out, hipStream_t stream) {
    const unsigned head = ((uintptr_t)out % 16 != 0) ? 1u : 0u;
    const size_t pairs = (n - head) / 2;
    const size_t blocks = std::min(std::max<size_t>((pairs + kIqThreads - 1) / kIqThreads, 1), kIqMaxBlocks);
    hipLaunchKernelGGL(k_iq_convert<FORMAT>, dim3((unsigned)blocks), dim3(kIqThreads), 0, stream,
                       static_cast<const typename IqFormat<FORMAT>::T*>(in), out, n, head);
    RC_HIP(hipGetLastError());
}

}  // namespace

bool iq_format_ok(int format) { return format == RCFM_IQ_CS16 || format == RCFM_IQ_CS8 || format == RCFM_IQ_CU8; }

void launch_iq_convert(int format, size_t n, const void* in, float2* out, hipStream_t stream) {
    RC_REQUIRE(iq_format_ok(format), RCFM_ERR_ARG, "unknown IQ format (RCFM_IQ_CS16, RCFM_IQ_CS8, RCFM_IQ_CU8)");
    if (n == 0) return;
    RC_REQUIRE(in && out, RCFM_ERR_ARG, "NULL argument");
    const size_t elem = format == RCFM_IQ_CS16 ? 2 : 1;
    RC_REQUIRE((uintptr_t)in % elem == 0 && (uintptr_t)out % sizeof(float2) == 0, RCFM_ERR_ARG,
               "misaligned buffer: `in` is aligned for one integer of the format, `out` for one complex64");
    switch (format) {
        case RCFM_IQ_CS16: launch_one<RCFM_IQ_CS16>(n, in, out, stream); break;
        case RCFM_IQ_CS8: launch_one<RCFM_IQ_CS8>(n, in, out, stream); break;
        default: launch_one<RCFM_IQ_CU8>(n, in, out, stream); break;
    }
}

}  // namespace rcfm

extern "C" {

int rcfm_iq_convert(int format, size_t n, const void* in, void* out_c64, void* stream) {
    return rcfm::guarded([&] {
        rcfm::launch_iq_convert(format, n, in, static_cast<float2*>(out_c64), rcfm::as_stream(stream));
    });
}

}  // extern "C"
