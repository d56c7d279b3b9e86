// IQ imbalance estimate and image rejection on the loaded spectrum (include/rcfm.h, rcfm_tuner_iq_*): how the kernels of
// iq_balance.hip split their work.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace rcfm {

constexpr int kIqBalThreads = 256;
constexpr int kIqSegPairs = 16384;    // mirror pairs per workgroup of k_iq_estimate (2 x 128 KiB of spectrum)
constexpr int kIqMaxSegs = 1024;      // ... and at most this many workgroups: the finish adds their sums in one thread
constexpr int kIqCorrectBlocks = 2048;   // k_iq_correct: at most this many workgroups, grid-stride beyond

// Workgroups of an estimate over `pairs` mirror pairs: a function of the pair count alone.
inline int iq_segments(int64_t pairs) {
    return (int)std::min<int64_t>(kIqMaxSegs, std::max<int64_t>((pairs + kIqSegPairs - 1) / kIqSegPairs, 1));
}

// X: bin 0 of the spectrum (the halos lie in front of it and behind bin n - 1).
// Estimate over mirror pairs m_lo .. m_hi (1 <= m_lo <= m_hi <= (n - 1) / 2): part [iq_segments(pairs)][3] float64 receives
// the workgroups' Re P, Im P, Q; the finishing launch adds them in order and writes sums [3] float64 and beta [2] float32
// (either may be null).
void launch_iq_estimate(const float2* X, int64_t n, int64_t m_lo, int64_t m_hi, double* part, double* sums, float* beta,
                        hipStream_t stream);
// In place: X[k] -= beta conj(X[(n - k) mod n]) for every bin, then the notch (bins of signed index |s| <= notch - 1 := 0),
// both halos rewritten.  beta: [2] float32 on the device.
void launch_iq_correct(float2* X, int64_t n, int64_t halo, const float* beta, int64_t notch, hipStream_t stream);

}  // namespace rcfm
