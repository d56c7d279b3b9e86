// The per-channel audio filter (include/rcfm.h, rcfm_audio_filter_*): how k_audio_filter of audio_filter.hip splits a row.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kSosMaxSections = 8;     // biquads of a filter
constexpr int kSosThreads = 256;       // one workgroup per channel; with two legs, 128 threads (two waves) per leg
constexpr int kSosRun = 33;            // R: samples of a leg one thread owns; odd, so that lanes a run apart hit different LDS banks
constexpr int kSosSegment = 8192;      // floats of a row that pass through LDS at a time: 8192 samples mono, 4096 frames stereo
constexpr int kSosPlanePad = 16;       // stereo lies in LDS as two planes, PlanePad floats further apart than their length:
                                       // the 4-byte staging of an unaligned row then writes both legs without a bank conflict
constexpr int kSosTables = 7;          // M^(R 2^k), k = 0 .. 5 (the scan inside a wave), and M^(64 R) (from wave to wave)

// What the kernel reads per section, built by rcfm_audio_filter_create in float64 (the powers in long double, rounded once).
// M = [[-a1, 1], [-a2, 0]] is the state's own map: z' = M z + (b1 - a1 b0, b2 - a2 b0) u.
struct SosSection {
    double b0, b1, b2, a1, a2;
    double pad_[3];
    double P[kSosTables][4];           // row-major 2 x 2
};

}  // namespace rcfm
