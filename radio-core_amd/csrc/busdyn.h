// Bus dynamics (include/rcfm.h, rcfm_busdyn_*): the limits of a handle and how the kernels of busdyn.hip deal a row out.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kBusdynMaxBuses = 1024;
constexpr int kBusdynMinBlock = 8;         // L: the block length, which is the look-ahead and the latency
constexpr int kBusdynMaxBlock = 2048;
constexpr int kBusdynMaxHold = 1 << 15;    // blocks of hang
constexpr int kBusdynMaxLength = 1 << 30;  // A_max
constexpr int kBusdynThreads = 256;        // peaks: four blocks per workgroup, one per wave; apply: 256 floats or vectors of a row
constexpr int kBusdynKnotThreads = 64;     // knots: one wave per bus, 64 knots at a time

}  // namespace rcfm
