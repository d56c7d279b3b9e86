// The frame gate (include/rcfm.h, rcfm_frame_power / rcfm_tuner_frame_levels / rcfm_gate_*): how the kernels of gate.hip
// split their rows.
#pragma once

#include <cstdint>

namespace rcfm {

constexpr int kGateThreads = 256;          // four waves: four short frames, or one segment of a long one
constexpr int kGateWaveFloats = 4096;      // a frame of up to this many floats (2 L for complex rows) belongs to ONE wave
constexpr int kGateSegFloats = 16384;      // longer frames: floats per workgroup (64 KB); more than one segment -> partial sums
constexpr int kGateMaxFrames = 65535;      // F of rcfm_gate_run / rcfm_gate_apply: one thread walks a channel's frames
constexpr int kGateMaxRamp = 1 << 20;      // R of rcfm_gate_create

// Segments of a frame of m floats: a function of m = L (1 + is_complex) alone.
inline int gate_segments(int64_t m) { return m <= kGateWaveFloats ? 1 : (int)((m + kGateSegFloats - 1) / kGateSegFloats); }

}  // namespace rcfm
