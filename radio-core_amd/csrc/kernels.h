// Launch wrappers of the hand-written gfx950 kernels (kernels.hip).
// All pointers are device pointers; all launches are asynchronous on `stream`.
#pragma once

#include "common.h"
#include "spectrum_rules.h"

namespace rcfm {

// Y[c][k] (m bins) <- roll + window + truncate/zero-pad of X[c][.] (n bins), complex
// spectra.  Shared by Tuner.run (tuner.py:159-161, x_stride = 0: every channel reads
// the same wideband spectrum) and complex Decimate (decimate.py:48).
//   wpos[k], k in [0, nyq): weight of source bin k; wneg[j], j in [1, nneg]: weight
//   of source bin n-j (wneg[0] unused); w_merge: weight of bin n - nmin/2 (NYQ_DOWN).
//   roll[c] in [0, n): Xrolled[k] = X[(k - roll) mod n]; may be null (no roll).
void launch_spectrum_c2c(const float2* X, int64_t x_stride, int64_t n, const int64_t* roll, float2* Y,
                         int64_t m, int batch, const float* wpos, const float* wneg, float w_merge,
                         int nyq, int nneg, int nyq_mode, float scale, hipStream_t stream);

// Half-spectrum version for real signals (FM/MFM audio decimation, real Decimate):
// X [batch][n/2+1] -> Y [batch][m/2+1]; wr = folded window; nyq_bin, nyq_factor: ResampleGeom.
void launch_spectrum_r2c(const float2* X, int64_t n, float2* Y, int64_t m, int batch, const float* wr,
                         int nyq, int nyq_bin, float nyq_factor, float scale, hipStream_t stream);

// Same resampling rule, but from the FULL complex spectrum X [batch][n] of a real signal to
// the full Hermitian spectrum Y [batch][m] (feeds a complex inverse FFT whose real part is y).
// dc (optional, [batch]): receives Y[c][0], the DC bin (sum of the resampled signal / m).
// paired: X is [ceil(batch/2)][n], one complex FFT per pair of real signals (x[2p] + j x[2p+1]).
void launch_spectrum_real_full(const float2* X, int64_t n, float2* Y, int64_t m, int batch, const float* wr,
                               int nyq, int nyq_bin, float nyq_factor, float scale, float2* dc, bool paired,
                               hipStream_t stream);

// scipy.signal.hilbert's mask (pll.py:34): P [batch][n/2+1] half spectrum of the real
// input -> Z [batch][n] one-sided spectrum {1, 2, ..., 2, 1, 0, ...} * scale.
void launch_hilbert_mask(const float2* P, float2* Z, int64_t n, int batch, float scale,
                         hipStream_t stream);

// WBFM audio decimation of both stereo legs at once (wbfm.py:86-87): U = FFT_B of the
// packed signal (m+lmr) + j(m-lmr); V [batch][A] = packed spectrum whose inverse FFT is
// l + j r, with the Hamming weight, truncation and Nyquist rule of decimate.py:48.
// dc (optional, [batch]): receives V[c][0] = (sum l, sum r) / A.
void launch_stereo_unpack(const float2* U, int64_t B, float2* V, int64_t A, int batch, const float* wr,
                          int nyq, int nyq_bin, float nyq_factor, float scale, float2* dc, hipStream_t stream);

// fm.py:60-65: d[0] = 0, d[i] = arg(x[i] conj(x[i-1])) / pi.
void launch_discriminator(const float2* iq, float* d, int64_t n, int batch, hipStream_t stream);

// Fused front end of WBFM.run (wbfm.py:77-80): discriminator -> same-size Decimate
// (3-tap circular Hamming, side tap = 0.23 or 0.23 cos(pi/n)) -> m; zero-phase pilot
// band-pass (filtfilt as a (2H+1)-tap symmetric FIR over an odd extension) -> p.
// g: H+1 taps, g[0] = centre.  iq != null: full chain.  iq == null: x is the FIR input
// (Bandpass.run primitive) and m_out is not written.
void launch_pilot_stage(const float2* iq, const float* x, float* m_out, float* p_out, int64_t n,
                        int batch, const float* g, int H, float side_tap, hipStream_t stream);

// Tile-blocked layout of the real signals m and p for readers that walk them as 16-line tiles of an L x R
// matrix (sample t = k R + i: the first pass of the pair FFT and the point-wise stage of k_fft_tile2_pair):
// element (k, i) of channel c sits at  c stride + (i / 16) bs + 16 k + i % 16  (bs >= 16 L),  so the 16 L values of a tile
// are one contiguous run instead of L 64-byte half lines R floats apart (each fetched as a whole line, half of
// them twice).  valid() = the pilot stage can write it: whole row PAIRS per workgroup (rpt rows, even), so that
// every 128-byte line (rows k, k + 1 of one 16-column block) leaves in one store instruction.
struct PilotBlocked {
    int R = 0, L = 0;       // row length (columns), rows: n = L R
    int rpt = 0, nb = 0;    // rows per workgroup (even, rpt R <= 2048), 16-column blocks per row
    int bs = 0;             // floats from one 16-column block to the next (>= 16 L)
    unsigned half_magic = 0;   // ceil(2^32 / (rpt / 2)): the stage's one division as a multiply-high
    int64_t stride = 0;     // floats per channel: nb * bs
    bool valid() const { return rpt > 0; }
    int blk16() const { return valid() ? bs : 0; }
    // the layout for an n = L R signal, or an invalid one when the stage would waste more than an eighth of its
    // threads (rpt R < 1792 of 2048), R is not a multiple of 4 (16-byte stores) or the signal is shorter than a workgroup
    static PilotBlocked plan(int64_t L, int64_t R);
};

// The same chain specialised for WBFM's 41-tap pilot filter (H = 40); g_host: 41 taps on the host.
// Needs n % 4 == 0 (16-byte stores) and n > 123.  blk (optional, valid()): m and p leave tile-blocked.
void launch_pilot_stage_h40(const float2* iq, float* m_out, float* p_out, int64_t n, int batch,
                            const float* g_host, float side_tap, hipStream_t stream, const PilotBlocked* blk = nullptr);
// The same chain from the samples' phases theta = angle(x) / pi (what the pipeline's tuner stage leaves,
// fused_tuner_ifft): d[i] = the phase step wrapped into [-1, 1], exactly diff(unwrap(angle(x))) / pi.
void launch_pilot_stage_h40_phase(const float* theta, float* m_out, float* p_out, int64_t n, int batch,
                                  const float* g_host, float side_tap, hipStream_t stream, const PilotBlocked* blk = nullptr);

// wbfm.py:83,86-87: s2 = Im(z^2)/|z^2|; lmr = s2 m 1.0175; u = (m + lmr) + j (m - lmr).
void launch_stereo_mix(const float2* z, const float* m, float2* u, size_t count, hipStream_t stream);

// pll.py:36-58 for arbitrary multiplier.
void launch_pll_phase(const float2* z, size_t count, double mult, int want_imag, float* out,
                      hipStream_t stream);

// Launch limits of the generic (any tap count, any batch) kernels; the entry points of rcfm.h check them on the host
// before anything is launched.  The batch index is a grid y / z coordinate (at most 65535).  The dynamic LDS of k_fir
// (2 nb + 1031 floats), k_fir_state (3 nb floats) and k_pilot_stage (5 H + 2051 floats, H = ntaps - 1) grows with the
// tap count and has to fit the 64 KiB a launch gets without asking for more: nb <= 5461 (k_fir_state binds; k_fir
// alone would take 7676) and H <= 2866.  kernels.hip asserts both against the tile sizes.
constexpr int kMaxBatch = 65535;
constexpr int kFirMaxTaps = 5461;
constexpr int kPilotMaxTaps = 2867;

// lfilter(taps, 1, x, zi=state) for an FIR (deemphasis.py:64).  x, y: [batch][n][ch]
// interleaved; state: [batch][ch][nb-1] transposed-direct-form-II state (read only).
// partial (optional): [batch][ch][fir_tiles(n)] per-tile sums of y for the DC removal.
int fir_tiles(int64_t n);
void launch_fir(const float* x, float* y, int64_t n, int ch, int batch, const float* taps, int nb,
                const float* state, float* partial, hipStream_t stream);
// The 51-tap de-emphasis case, register-blocked (n*ch % 4 == 0 for its 16-byte stores);
// partial: [batch][fir51_tiles(n, ch)] (both stereo legs share a tile).  taps_host: 51 floats.
int fir51_tiles(int64_t n, int ch);
// dc != nullptr ([batch], from launch_stereo_unpack / launch_spectrum_real_full): the kernel also
// removes the mean and clips (mfm.py:64-65, wbfm.py:97-100); `partial` is then unused.  Needs n >= 50.
// row_samples / row_pitch_samples (fir51 and fir_state): the input signal is stored in rows of row_samples samples at a
// pitch of row_pitch_samples (0 = contiguous): the padded output of fused_fft_decim_ifft.
void launch_fir51(const float* x, float* y, int64_t n, int ch, int batch, const float* taps_host,
                  const float* state, float* partial, const float2* dc, hipStream_t stream, int row_samples = 0,
                  int row_pitch_samples = 0);
// Advance `state` to the end of the buffer (must run after launch_fir on the stream).
void launch_fir_state(const float* x, int64_t n, int ch, int batch, const float* taps, int nb,
                      float* state, hipStream_t stream, int row_samples = 0,
                      int row_pitch_samples = 0);
// mfm.py:64-65 / wbfm.py:97-100: y -= mean(y) over the channel's n*ch samples; clip +-0.999.
// partial: [batch][nparts] partial sums of y.
void launch_dc_clip(float* y, int64_t n, int ch, int batch, const float* partial, int nparts,
                    hipStream_t stream);

// AM (RCFM_AM): e = |x| of n complex samples (iq [n] complex64 -> e [n] float32; a batch of channels is one flat run).
// 16-byte accesses when both pointers are 16-byte aligned.
void launch_envelope(const float2* iq, float* e, int64_t n, hipStream_t stream);
// AM's tail, in place on y [batch][n]: y = clip(y / c - 1, +-0.999) with c = the channel's mean, zeros when !(c > 0).
// dc != nullptr ([batch], from launch_spectrum_real_full / the decimating tile): c = dc[c].x, the DC bin of the
// resampled spectrum (= the mean of y); else every channel reduces its own y first.
void launch_am_tail(float* y, int64_t n, int batch, const float2* dc, hipStream_t stream);

// SSB (RCFM_USB / RCFM_LSB) between rocFFT's transforms: full spectra X [batch][n] of the channel samples -> half
// spectra Y [batch][m / 2 + 1] of the resampled sideband signal (bins 1 .. kmax of the upper, or mirrored lower, half;
// wr, nyq_bin / nyq_factor and scale as in launch_spectrum_r2c).
void launch_ssb_select(const float2* X, int64_t n, float2* Y, int64_t m, int batch, const float* wr, int kmax,
                       int nyq_bin, float nyq_factor, float scale, bool lower, hipStream_t stream);
// SSB's tail, in place on y [batch][n]: y = clip(level y / g, +-0.999) with g = the channel's RMS, zeros when !(g > 0).
// One workgroup per channel and a fixed summation order: bit-identical from run to run.
void launch_ssb_tail(float* y, int64_t n, int batch, float level, hipStream_t stream);

// Per-channel signal level (rcfm_tuner_levels): power[c] = sum_k |Y_c[k]|^2 / N^2 over the B_c bins channel c reads from
// the wideband spectrum X (bin 0 of it), Y_c as launch_spectrum_c2c with the Hann weight builds it (NYQ_DOWN merge
// included) -- by Parseval the mean |x|^2 of the channel's samples, without the inverse FFT.  bw [count]: B_c <= N;
// the channels may differ in bandwidth.
//   base != nullptr (fast form): X is haloed, the run of channel c is X[base[c] - (B_c - 1) / 2 .. base[c] + B_c / 2]
//     with no wrap-around, read 16 bytes per lane; the window is the 4-term series of the tuner's fast gather.
//   base == nullptr (general form): bin (d - roll[c]) mod N per element, 64-bit, library cosine.
// A channel is split into level_segments(B_c) workgroups, a function of B_c alone; part ([count][max segments] float64,
// needed when any channel has more than one) receives their sums and a finishing launch adds them in segment order:
// bit-identical from run to run.
int level_segments(int64_t B);
void launch_channel_levels(const float2* X, int64_t N, const int32_t* base, const int64_t* roll, const int32_t* bw,
                           int count, int max_segments, double* part, float* power, hipStream_t stream);
// Carrier estimates (rcfm_tuner_carriers): over the B_c bins of channel c at signed offsets d = -(B_c / 2) ..
// -(B_c / 2) + B_c - 1 of its centre, p_d = |X[(d - roll[c]) mod N]|^2 in float64, unweighted:
//   peak_bin[c] = the d of the largest p_d (the lowest d among equals; a NaN never wins), peak_power[c] = that p_d / N^2,
//   centroid[c] = S1 / S0, spread[c] = sqrt(max(S2 / S0 - (S1 / S0)^2, 0)), S_k = sum of d^k p_d over the bins with
//   p_d >= gate_n2 (both 0 when S0 is not positive).  Any output may be null.
//   base != nullptr (fast form): X is haloed, the run of channel c is X[base[c] - B_c / 2 .. ] with no wrap-around, read
//     16 bytes per lane;  base == nullptr (general form): bin (d - roll[c]) mod N per element, 64-bit.
// Segments as launch_channel_levels: level_segments(B_c) workgroups per channel; part ([count][max segments], needed when
// any channel has more than one) receives their records and a finishing launch combines them in segment order:
// bit-identical from run to run, and whichever outputs are null.
struct CarrierPart {
    double s0, s1, s2, mx;
    int32_t md, pad;
};
void launch_channel_carriers(const float2* X, int64_t N, const int32_t* base, const int64_t* roll, const int32_t* bw,
                             int count, int max_segments, double gate_n2, CarrierPart* part, int32_t* peak_bin,
                             float* peak_power, float* centroid, float* spread, hipStream_t stream);
// Wideband power spectrum (rcfm_tuner_power_spectrum): the span of L signed bins from s0 (bin s = X[s mod N]; it does not
// wrap in frequency) is cut into M cells, cell m = span positions [floor(m L / M), floor((m + 1) L / M));
// power[m] = sum, peak[m] = max of |X|^2 / N^2 over the cell, float64 inside, float32 out; either may be null.
// Cells of at most 16 bins take a thread each, of at most 1024 bins a wave each; longer ones power_segments(L, M)
// workgroups each -- all functions of (L, M) alone.  part_sum ([M][segments] float64) and part_max ([M][segments] float32),
// needed when power_segments > 1, receive the segments' results and a finishing launch combines them in segment order:
// bit-identical from run to run.
int power_segments(int64_t L, int64_t M);
void launch_power_spectrum(const float2* X, int64_t N, int64_t s0, int64_t L, int64_t M, double* part_sum, float* part_max,
                           float* power, float* peak, hipStream_t stream);
// Squelch (rcfm_squelch): open[c] = power[c] >= threshold[c] (false for NaN), one byte per channel (open may be null);
// rows of closed channels of audio [count][row] float32 (may be null) := 0, rows of open channels untouched.
void launch_squelch(const float* power, const float* threshold, int count, size_t row, float* audio, uint8_t* open,
                    hipStream_t stream);
// Raw integer IQ (iq.hip; include/rcfm.h, RCFM_IQ_*): n interleaved pairs at `in` (aligned for one integer) -> out [n]
// complex64, each value exactly the format's integer times its power of two.  n = 0: nothing is launched.
bool iq_format_ok(int format);
void launch_iq_convert(int format, size_t n, const void* in, float2* out, hipStream_t stream);

}  // namespace rcfm
