// Stateful AGC tail (include/rcfm.h, rcfm_agc / rcfm_demod_set_agc): how k_agc_tail of agc.hip walks one row.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rcfm {

constexpr int kAgcThreads = 256;     // one workgroup per row
constexpr int kAgcSegment = 8192;    // samples of a row staged in LDS at a time (32 KiB): A = 8000 is one segment

// Samples per thread of a segment of `len` samples: thread t owns the contiguous run [t R, (t + 1) R).  R is odd, so lanes
// a run apart read 32 different LDS banks.  A function of len alone -- and len of n alone --, so the order of every
// operation is too.
constexpr int agc_run(int len) { return ((len + kAgcThreads - 1) / kAgcThreads) | 1; }

// What a caller sets (the entry points have checked it: decay_samples > 0, level > 0, floor >= 0, all finite).
struct AgcParams {
    double decay_samples;
    float level, floor;
};
inline AgcParams agc_params(double decay_samples, float level, float floor) { return AgcParams{decay_samples, level, floor}; }

// v [batch][n] -> audio [batch][n] (audio == v allowed, no other overlap), state [batch] float32 in/out.
// mode: RCFM_AGC_PEAK or RCFM_AGC_CARRIER.
void launch_agc_tail(int mode, const float* v, float* audio, int64_t n, int batch, const AgcParams& p, float* state,
                     hipStream_t stream);

}  // namespace rcfm
