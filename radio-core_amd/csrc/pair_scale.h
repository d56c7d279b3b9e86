// Per-row power-of-two scaling of AM / SSB channels that share a complex transform (pair_scale.hip).
//
// On the FFT-engine routes AM and SSB carry two channels in one complex transform (AM: the envelopes of rows 2P and
// 2P + 1 as real and imaginary part; SSB: Y0 + j Y1 into the inverse transform).  A float32 transform rounds at the scale
// of its larger member, and unlike the FM family -- which pairs discriminator output, level-free by construction --
// these two pair signals at the stations' own RF levels.  So each row gets a factor 2^e that brings its largest
// magnitude into [1, 2) before the shared transform.  A power of two is exact: without AGC it cancels in the tails'
// division by the row's own mean / RMS; with AGC launch_rows_rescale takes it out again before the follower sees the
// signal, so the carried state keeps its absolute units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rcfm {

constexpr int kPairScaleThreads = 256;   // one workgroup per row

// scale [2][rows]: scale[r] = 2^e of row r, scale[rows + r] = 2^-e.  A row that is all zero, or whose largest magnitude
// is not finite, keeps the factor 1.

// AM: e [rows][n] real rows (the envelopes), scaled in place.
void launch_am_pair_scale(float* e, int64_t n, int rows, float* scale, hipStream_t stream);

// SSB: the factors alone (LoadSsbPairT applies them on the load), from the largest |re|, |im| of the sideband bins
// 1 .. kmax of each channel: X and base32 as in SsbSource (fused_passes.h).
void launch_ssb_pair_scale(const float2* X, const int32_t* base32, int B, int kmax, bool lower, int rows, float* scale,
                           hipStream_t stream);

// y [rows][n] *= factor[r], in place.
void launch_rows_rescale(float* y, int64_t n, int rows, const float* factor, hipStream_t stream);

}  // namespace rcfm
