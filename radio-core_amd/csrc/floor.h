// The noise floor (include/rcfm.h, rcfm_rank_filter / rcfm_floor_*): how the kernel of floor.hip tiles the cells, and the
// ordering of float32 values every rank is taken in.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kFloorThreads = 256;         // one cell per thread: a workgroup owns 256 cells and reads 256 + 2 half keys
constexpr int kFloorMaxHalf = 4096;        // (256 + 8192) keys: 33 KB of LDS at the most
constexpr int64_t kFloorMaxCells = (int64_t)1 << 30;
constexpr uint32_t kFloorNaN = 0x7fc00000u;   // the NaN that is stored, and the state of a cell that is not primed

}  // namespace rcfm
