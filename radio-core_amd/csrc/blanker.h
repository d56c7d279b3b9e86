// The wideband noise blanker (include/rcfm.h, "noise blanker"; rcfm_blanker_*): how the kernels of blanker.hip split their
// work.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kBlankThreads = 256;
constexpr int kBlankTile = 4096;                    // samples per workgroup of every pass: 128 whole mask words
constexpr int kBlankTileWords = kBlankTile / 32;
constexpr int kBlankWaveRun = kBlankTile / (kBlankThreads / 64);   // consecutive samples of a tile one wave takes (1024)
constexpr int kBlankMaxGuard = 1024;                // G = hold + ramp at most: 32 mask words each side of a tile
constexpr int kBlankHaloWords = kBlankMaxGuard / 32;
constexpr int kBlankWindowWords = kBlankTileWords + 2 * kBlankHaloWords;   // 192 words in LDS
constexpr int kBlankMinBlock = 64, kBlankMaxBlockLog2 = 20;
constexpr int kBlankMaxSpan = 8;
constexpr int64_t kBlankMaxSamples = (int64_t)1 << 40;

inline int64_t blank_tiles(int64_t n) { return (n + kBlankTile - 1) / kBlankTile; }

}  // namespace rcfm
