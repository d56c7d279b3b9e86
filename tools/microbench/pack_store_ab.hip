// Microbenchmark: the pack kernel of rcfm_audio_pack (radio-core_amd/csrc/egress_kernel.h, the kernel the library launches)
// with plain and with non-temporal stores, at the cfg4 audio geometry (1024 channels x 96 000 floats), every channel open
// and one in ten open, next to a device-to-device copy of the same number of bytes read plus written.  Alternating rounds.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../include -I../../radio-core_amd/csrc -o pack_store_ab pack_store_ab.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "egress_kernel.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

using namespace rcfm;

constexpr int kCount = 1024;
constexpr size_t kRow = 96000;

template <int FORMAT, bool NT>
void pack(const float* audio, const int32_t* slot, void* packed) {
    const dim3 grid(kCount, (unsigned)((kRow + kPackSegment - 1) / kPackSegment), 1);
    hipLaunchKernelGGL((k_audio_pack<FORMAT, true, NT>), grid, dim3(kPackThreads), 0, 0, audio, slot, kRow, 32767.0f, packed);
}

template <class F>
float timed(F launch) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    CK(hipEventRecord(a));
    launch();
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float ms;
    CK(hipEventElapsedTime(&ms, a, b));
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    return ms;
}

int main() {
    const size_t floats = (size_t)kCount * kRow;
    float* audio;
    void* packed;
    char* scratch;
    uint8_t* open;
    int32_t *slot_all, *slot_tenth;
    CK(hipMalloc(&audio, floats * 4));
    CK(hipMalloc(&packed, floats * 4));
    CK(hipMalloc(&scratch, floats * 4));
    CK(hipMalloc(&open, kCount));
    CK(hipMalloc(&slot_all, kCount * 4));
    CK(hipMalloc(&slot_tenth, kCount * 4));
    std::vector<float> h(floats);
    unsigned s = 12345;
    for (auto& v : h) {
        s = s * 1664525u + 1013904223u;
        v = ((float)(s >> 8) / 8388608.0f - 1.0f) * 0.9f;
    }
    CK(hipMemcpy(audio, h.data(), floats * 4, hipMemcpyHostToDevice));
    std::vector<uint8_t> m(kCount);
    int n_tenth = 0;
    for (int c = 0; c < kCount; ++c) n_tenth += (m[c] = c % 10 == 3);
    CK(hipMemcpy(open, m.data(), kCount, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_slot_scan, dim3(1), dim3(kScanThreads), 0, 0, (const uint8_t*)nullptr, kCount, slot_all, (int32_t*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_slot_scan, dim3(1), dim3(kScanThreads), 0, 0, (const uint8_t*)open, kCount, slot_tenth, (int32_t*)nullptr, (int32_t*)nullptr);
    CK(hipDeviceSynchronize());

    struct Case {
        const char* name;
        double bytes;          // read + written
        std::vector<float> ms;
    };
    const double all16 = floats * 6.0, all32 = floats * 8.0, t16 = (double)n_tenth * kRow * 6.0, t32 = (double)n_tenth * kRow * 8.0;
    std::vector<Case> cases = {{"s16 all open, plain", all16, {}},   {"s16 all open, non-temporal", all16, {}},
                               {"f32 all open, plain", all32, {}},   {"f32 all open, non-temporal", all32, {}},
                               {"s16 10% open, plain", t16, {}},     {"s16 10% open, non-temporal", t16, {}},
                               {"f32 10% open, plain", t32, {}},     {"f32 10% open, non-temporal", t32, {}},
                               {"d2d copy, bytes of s16 all", all16, {}}, {"d2d copy, bytes of f32 all", all32, {}},
                               {"d2d copy, bytes of s16 10%", t16, {}},   {"slot scan, 1024 channels", 0.0, {}},
                               {"slot scan, 65535 channels", 0.0, {}}};
    uint8_t* open_big;
    int32_t* slot_big;
    CK(hipMalloc(&open_big, 65535));
    CK(hipMalloc(&slot_big, 65535 * 4));
    CK(hipMemset(open_big, 1, 65535));
    for (int round = 0; round < 12; ++round) {
        std::vector<float> t = {
            timed([&] { pack<RCFM_PCM_S16, false>(audio, slot_all, packed); }),
            timed([&] { pack<RCFM_PCM_S16, true>(audio, slot_all, packed); }),
            timed([&] { pack<RCFM_PCM_F32, false>(audio, slot_all, packed); }),
            timed([&] { pack<RCFM_PCM_F32, true>(audio, slot_all, packed); }),
            timed([&] { pack<RCFM_PCM_S16, false>(audio, slot_tenth, packed); }),
            timed([&] { pack<RCFM_PCM_S16, true>(audio, slot_tenth, packed); }),
            timed([&] { pack<RCFM_PCM_F32, false>(audio, slot_tenth, packed); }),
            timed([&] { pack<RCFM_PCM_F32, true>(audio, slot_tenth, packed); }),
            timed([&] { CK(hipMemcpyAsync(scratch, audio, (size_t)(all16 / 2), hipMemcpyDeviceToDevice, 0)); }),
            timed([&] { CK(hipMemcpyAsync(scratch, audio, (size_t)(all32 / 2), hipMemcpyDeviceToDevice, 0)); }),
            timed([&] { CK(hipMemcpyAsync(scratch, audio, (size_t)(t16 / 2), hipMemcpyDeviceToDevice, 0)); }),
            timed([&] { hipLaunchKernelGGL(k_slot_scan, dim3(1), dim3(kScanThreads), 0, 0, (const uint8_t*)open, kCount, slot_tenth, (int32_t*)nullptr, (int32_t*)nullptr); }),
            timed([&] { hipLaunchKernelGGL(k_slot_scan, dim3(1), dim3(kScanThreads), 0, 0, (const uint8_t*)open_big, 65535, slot_big, (int32_t*)nullptr, (int32_t*)nullptr); })};
        if (round >= 2)   // two warm-up rounds
            for (size_t i = 0; i < cases.size(); ++i) cases[i].ms.push_back(t[i]);
    }
    CK(hipGetLastError());
    printf("%-30s %10s %10s %10s %9s\n", "case (10 alternating rounds)", "median us", "min us", "max us", "TB/s");
    for (auto& c : cases) {
        std::sort(c.ms.begin(), c.ms.end());
        const double med = 0.5 * (c.ms[4] + c.ms[5]);
        printf("%-30s %10.1f %10.1f %10.1f %9.2f\n", c.name, med * 1e3, c.ms.front() * 1e3, c.ms.back() * 1e3, c.bytes / (med * 1e-3) / 1e12);
    }
    return 0;
}
