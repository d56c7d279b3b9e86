// Audio buses (include/rcfm.h, rcfm_mix_*): the limits of a mixer and how the kernel of mix.hip deals a bus out.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kMixMaxBuses = 1024;
constexpr int kMixMaxBusRoutes = 65535;
constexpr int kMixMaxRoutes = 1 << 20;
constexpr int kMixSegment = 16;            // routes of one segment sum: part of the definition, not a tuning knob
constexpr int kMixWaves = 16;              // a workgroup takes this many segments of a bus at a time, one per wave
constexpr int kMixThreads = 64 * kMixWaves;
constexpr int kMixTile = 256;              // samples of a bus row per workgroup: four per lane
constexpr int kMixBatch = 8;               // open routes whose row loads a wave issues before it adds them, in order

}  // namespace rcfm
