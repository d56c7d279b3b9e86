// The tone bank (include/rcfm.h, rcfm_tone_bank_* and rcfm_tone_score): how the kernels of tones.hip split their work.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kToneMaxK = 64;          // tones of a bank
constexpr int kToneMaxL = 1 << 24;     // frame length: the coarse table holds K ceil(L / kToneChunk) complex64
constexpr int kToneBlock = 8;          // tones per wave: 16 float accumulators per lane
constexpr int kToneChunk = 16;         // J: samples a lane takes at a time, exp(-2 pi j nu (m J + j)) = coarse[k][m] fine[k][j]
constexpr int kToneChunkPad = 20;      // floats between chunks in LDS: 16-byte reads of 64 lanes touch every bank once
constexpr int kToneSegChunks = 512;    // chunks per workgroup: eight per lane
constexpr int kToneSegment = kToneSegChunks * kToneChunk;   // samples of a frame per workgroup (8192: 40 KiB of LDS)
constexpr int kToneScoreThreads = 256;

// Workgroups a frame of L samples is split over: a function of L alone.  One segment writes P and E itself; several
// leave float partial sums that the finish adds in segment order.
inline int tone_segments(int L) { return (L + kToneSegment - 1) / kToneSegment; }
// Waves of a workgroup (one per block of kToneBlock tones) and the tone count padded to whole blocks.
inline int tone_waves(int K) { return (K + kToneBlock - 1) / kToneBlock; }
inline int tone_padded(int K) { return tone_waves(K) * kToneBlock; }
inline int tone_chunks(int L) { return (L + kToneChunk - 1) / kToneChunk; }

}  // namespace rcfm
