// Subcarrier tap (include/rcfm.h, rcfm_subcarrier_*): how the kernel of subcarrier.hip tiles one channel.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kTapBlock = 4;                  // consecutive outputs per thread = taps per step of the inner loop
constexpr int kTapThreads = 256;               // per workgroup: all of them stage, the first J / 4 compute
constexpr int kTapStageBatch = 4;              // 4-sample groups a thread has in flight while it stages
constexpr int kTapWideLds = 32 * 1024;        // tiles of whole waves stay below it: several workgroups per CU
constexpr int kTapMaxLds = 64 * 1024;

// The tile of k_subcarrier_tap for decimation D and T taps -- a function of (D, T) alone, so the order of every sum is too.
//   J     outputs per workgroup (0: no tile fits 64 KiB; k_subcarrier_tap_single computes one output per workgroup)
//   rpad  taps per polyphase component, zero-padded to whole steps: ceil(ceil(T / D) / 4) * 4
//   Q     floats per component row in LDS: J + rpad + 4 (the inner loop reads one step ahead)
struct TapTile {
    int J = 0, rpad = 0, Q = 0;
    size_t lds_bytes(int D) const { return sizeof(float) * (size_t)D * (size_t)Q; }
};

inline TapTile tap_tile(int D, int T) {
    TapTile t;
    t.rpad = ((int)(((int64_t)T + D - 1) / D) + kTapBlock - 1) / kTapBlock * kTapBlock;   // (T + D in 64 bits: D reaches 2^31 - 1)
    for (int J : {1024, 512, 256, 128, 64, 32, 16, 8, 4}) {
        t.J = J;
        t.Q = J + t.rpad + kTapBlock;
        if (t.lds_bytes(D) <= (size_t)(J > 256 ? kTapWideLds : kTapMaxLds)) return t;
    }
    t.J = t.Q = 0;
    return t;
}

// y [count][R] from phases (from_phase: in = float32 [count][B], angle / pi) or samples (complex64 [count][B]).
// g: T taps; gp: the same taps by polyphase component [min(D, T)][rpad]; rot: [R].
void launch_subcarrier_tap(const void* in, bool from_phase, float2* out, const float2* g, const float2* gp, const float2* rot,
                           int B, int R, int T, int count, hipStream_t s);

}  // namespace rcfm
