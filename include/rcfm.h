/*
 * rcfm.h -- C ABI of librcfm.so: the MI355X (gfx950) implementation of
 * radio-core's per-buffer DSP hot path (Tuner -> FM / MFM / WBFM).
 *
 * The reference (luigifcruz/radio-core v1.0.0) has no FFI: its device seam is
 * the module swap in radiocore/_internal/injector.py:16-29 (numpy+scipy vs
 * cupy+cusignal).  This header is what a third Injector branch binds instead
 * (INTEGRATION.md shows the ctypes stub).  Every entry point names the
 * reference call site(s) it replaces, relative to the reference checkout.
 *
 * Conventions
 *   - plain C types only; all data pointers are DEVICE pointers unless the
 *     parameter name ends in _host;
 *   - complex data is interleaved float (re, im) = numpy complex64;
 *   - every function returns 0 on success or a negative rcfm_status;
 *     rcfm_last_error() gives the message of the calling thread's last failure;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls
 *     are asynchronous on that stream; handles are not thread-safe (the
 *     reference is driven by one DSP thread, examples/multi_fm_server.py:86-106);
 *   - inputs are never modified; outputs are caller-owned; state and
 *     workspaces are owned by the handle and released by *_destroy.
 *   - the library reads ONE environment variable, once per process: RCFM_FFT=rocfft
 *     routes every transform through rocFFT (safety net and A/B partner; the
 *     default is the hand-written engine, rocFFT only for lengths outside it).
 *     Every other choice is an argument or a *_set_option of a handle;
 *   - this header is what a HOST binds (tuner, demodulators, pipeline, ingest, gather, primitives, plain FFT).  The
 *     entry points that exist for the repo's own tools and tests -- placement arenas, explicit FFT plans, the
 *     kernel-form switches, per-stage profiling -- are declared in rcfm_tools.h (same library, same conventions);
 *   - batched arrays are channel-major and contiguous: iq [C][B] complex64,
 *     audio [C][A][ch] float32 (ch = 1 for FM/MFM, 2 = interleaved L,R for WBFM,
 *     the byte layout of the reference's (1, A, 2) array, wbfm.py:94).
 */
#ifndef RCFM_H
#define RCFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCFM_VERSION 102 /* 0.1.2: tooling entry points moved to rcfm_tools.h (same symbols), RCFM_OPT_GRAPH;
                            demodulator kinds RCFM_AM, RCFM_USB, RCFM_LSB (no new entry points);
                            rcfm_tuner_levels and rcfm_squelch added (new symbols only, nothing existing changed);
                            rcfm_tuner_power_spectrum added (a new symbol only, nothing existing changed);
                            rcfm_tuner_carriers and rcfm_tuner_retune added (new symbols only, nothing existing changed);
                            rcfm_subcarrier_* and rcfm_pipeline_subcarrier added (new symbols only, nothing existing changed);
                            rcfm_agc, rcfm_demod_set_agc and rcfm_demod_get / set_agc_state added (new symbols only; a handle
                            that never calls rcfm_demod_set_agc launches what it launched before);
                            rcfm_tuner_load_raw and rcfm_iq_convert added (new symbols only; rcfm_tuner_load launches what it
                            launched before);
                            rcfm_audio_pack and rcfm_drain_* added (new symbols only, nothing existing changed);
                            rcfm_tuner_iq_estimate, rcfm_tuner_iq_correct and rcfm_tuner_set_iq_balance added (new symbols
                            only; a handle that never calls rcfm_tuner_set_iq_balance launches what it launched before);
                            rcfm_tone_bank_* and rcfm_tone_score added (new symbols only, nothing existing changed; a frame
                            length above 2^24 is refused: an implementation limit, the definition itself has none);
                            rcfm_audio_filter_* added (new symbols only, nothing existing changed);
                            rcfm_subcarrier_describe added to rcfm_tools.h (a new host-only symbol, nothing existing changed);
                            rcfm_blanker_* added, rcfm_blanker_last in rcfm_tools.h, RCFM_IQ_CF32 = 0 named (new symbols only,
                            nothing existing changed: the load entry points refuse format 0 as before);
                            rcfm_rank_filter and rcfm_floor_* added (new symbols only, nothing existing changed);
                            rcfm_mix_* added (new symbols only, nothing existing changed);
                            rcfm_busdyn_* added, rcfm_busdyn_state in rcfm_tools.h (new symbols only, nothing existing changed) */

typedef enum rcfm_status {
    RCFM_OK = 0,
    RCFM_ERR_SIZE = -1,    /* -> ValueError("input_sig size and input_size mismatch") fm.py:57-58 */
    RCFM_ERR_INDEX = -2,   /* -> IndexError (bad channel index, tuner.py:151) */
    RCFM_ERR_RUNTIME = -3, /* HIP / rocFFT failure */
    RCFM_ERR_ARG = -4,     /* invalid argument (NULL handle, unsupported size, ...) */
    RCFM_ERR_STATE = -5    /* call order (tuner_run before tuner_load, tuner.py:140-161) */
} rcfm_status;

typedef enum rcfm_demod_kind {
    RCFM_FM = 0,  /* radiocore/analog/fm.py:26-72   */
    RCFM_MFM = 1, /* radiocore/analog/mfm.py:29-71  */
    RCFM_WBFM = 2, /* radiocore/analog/wbfm.py:32-105 */
    /* AM envelope detector (no reference counterpart), one audio channel, no state; tau is ignored.  Per channel and
       buffer, float32: e = |x| (B samples); v = Decimate(B -> A)(e), the same periodic-Hamming resample as FM;
       c = mean(v), the carrier level; audio = clip(v / c - 1, -0.999, 0.999), or zeros when !(c > 0). */
    RCFM_AM = 3,
    /* Single sideband (no reference counterpart), one audio channel, no state; tau is ignored.  The channel centre is the
       suppressed carrier.  Per channel and buffer, for the B channel samples x:
         X = fft(x);  H_usb[k] = 2 for 1 <= k <= (B-1)/2, else 0 (DC and, for even B, the bin B/2 are dropped);
         H_lsb[k] = H_usb[(B - k) mod B];  s = Re(ifft(H X));  v = Decimate(B -> A)(s), the resample FM and AM use;
         g = sqrt(mean(v^2));  audio = clip(RCFM_SSB_LEVEL v / g, -0.999, 0.999), or zeros when !(g > 0).
       The per-buffer RMS normalisation makes the audio level independent of the station's level.
       Value 4 is unassigned: rcfm_demod_create refuses it (and everything above 6) as an unknown kind. */
    RCFM_USB = 5,
    RCFM_LSB = 6
} rcfm_demod_kind;

/* Audio RMS of a USB / LSB channel: a single tone peaks at 0.354, Gaussian noise reaches the clip at 4 sigma. */
#define RCFM_SSB_LEVEL 0.25f

typedef struct rcfm_tuner_s* rcfm_tuner_t;
typedef struct rcfm_demod_s* rcfm_demod_t;
typedef struct rcfm_subcarrier_s* rcfm_subcarrier_t;
typedef struct rcfm_tone_bank_s* rcfm_tone_bank_t;
typedef struct rcfm_audio_filter_s* rcfm_audio_filter_t;
typedef struct rcfm_gate_s* rcfm_gate_t;
typedef struct rcfm_floor_s* rcfm_floor_t;
typedef struct rcfm_mix_s* rcfm_mix_t;
typedef struct rcfm_busdyn_s* rcfm_busdyn_t;
typedef struct rcfm_resampler_s* rcfm_resampler_t;
typedef struct rcfm_feeder_s* rcfm_feeder_t;
typedef struct rcfm_comm_s* rcfm_comm_t;

/* ---- library / device ---------------------------------------------------- */

int rcfm_version(void);
const char* rcfm_last_error(void);
/* replaces radiocore.HasCuda() (radiocore/__init__.py:6-26): number of HIP devices */
int rcfm_device_count(int* count);
/* Plain device-memory helpers for hosts that do not bring their own allocator
 * (replace cupy.asarray / cupy.asnumpy at tuner.py:137, fm.py:60,70). */
int rcfm_malloc(void** dptr, size_t bytes);
int rcfm_free(void* dptr);
int rcfm_memcpy_h2d(void* dst, const void* src_host, size_t bytes, void* stream);
int rcfm_memcpy_d2h(void* dst_host, const void* src, size_t bytes, void* stream);
int rcfm_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int rcfm_stream_sync(void* stream);
/* A stream of the host's own for hosts without a HIP header (examples/c_host.c runs two lanes, RCFM_OPT_STATE_FENCE below):
 * hipStreamCreateWithFlags(hipStreamNonBlocking) / hipStreamDestroy.  Every `void* stream` argument of this header takes
 * one (or any hipStream_t, or NULL for the default stream). */
int rcfm_stream_create(void** stream);
int rcfm_stream_destroy(void* stream);

/* ---- Tuner (radiocore/tools/tuner.py) ------------------------------------ */

/* Tuner geometry is host-side Python in both trees (tuner.py:77-124,163-174);
 * the device handle receives the result: n = int(input_bandwidth) wideband
 * samples per buffer, and per channel roll[c] = int(f_in - f_c) (tuner.py:152)
 * and bw[c] = int(bandwidth) (tuner.py:153). */
int rcfm_tuner_create(int64_t n, int nch, const int64_t* roll_host, const int32_t* bw_host,
                      rcfm_tuner_t* out);
/* Tuner.load, tuner.py:126-138: X = FFT_n(x), kept by the handle. x: [n] complex64. */
int rcfm_tuner_load(rcfm_tuner_t t, const void* x, void* stream);
/* Raw integer IQ as receivers deliver it (no reference counterpart: the reference's load takes complex64 only): n pairs
 * interleaved I, Q, little-endian, full scale 1.0.  Every conversion is exact in float32:
 *   RCFM_IQ_CS16  int16  (Airspy, the USRP wire format, most files)   (float)i * 2^-15
 *   RCFM_IQ_CS8   int8   (HackRF)                                     (float)i * 2^-7
 *   RCFM_IQ_CU8   uint8  (RTL-SDR; the centre is 127.5)               ((float)u - 127.5f) * 2^-7   (255 -> 0.99609375) */
enum { RCFM_IQ_CS16 = 1, RCFM_IQ_CS8 = 2, RCFM_IQ_CU8 = 3 };
/* The fourth value of the same enumeration, complex64 itself: a format of rcfm_blanker_run only -- rcfm_tuner_load_raw and
 * rcfm_iq_convert refuse it like any other value they do not convert. */
enum { RCFM_IQ_CF32 = 0 };
/* rcfm_tuner_load of a raw buffer, x: [n][2] of the format's integer type on the device: the spectrum (halos, shard window,
 * held bins) is bit for bit that of rcfm_tuner_load of the converted samples, and the same refusals apply.  Where the
 * handle's wideband FFT runs on the engine, the conversion rides on the first pass's load (the buffer is read once, at 4
 * or 2 bytes per sample, and complex64 samples never exist in memory); otherwise (lengths that run on rocFFT,
 * RCFM_FFT=rocfft) rcfm_iq_convert fills a scratch buffer of the handle, reserved by the first such load, and the
 * complex64 load runs on that.  Any other format: RCFM_ERR_ARG before any device call. */
int rcfm_tuner_load_raw(rcfm_tuner_t t, int format, const void* x, void* stream);
/* The conversion alone, for hosts that feed rcfm_resampler_run / rcfm_demod_run or code of their own: n pairs at `in`
 * (device memory, aligned for one integer of the format -- not for a pair) -> out_c64 [n] complex64.  n = 0 is a no-op. */
int rcfm_iq_convert(int format, size_t n, const void* in, void* out_c64, void* stream);
/* Multi-GPU sharding (no reference counterpart: the reference has one device; its loop over all channels is
 * examples/multi_fm_server.py:100-106).  A rank that will only run channels [first, first + count) declares
 * it before rcfm_tuner_load: the last pass of the wideband FFT then stores only the part of the spectrum
 * those channels read (the other bins of the kept spectrum are undefined).  Default: every channel.
 * rcfm_tuner_run / rcfm_pipeline_run remember the range that was in force at load time and fail with
 * RCFM_ERR_STATE for a channel outside it; a new range takes effect with the next rcfm_tuner_load. */
int rcfm_tuner_shard(rcfm_tuner_t t, int first, int count);
/* Tuner.run for channels [first, first+count), tuner.py:140-161: circular shift
 * by roll, fftshifted-Hann weight, brick-wall truncation to bw bins, inverse
 * FFT, x bw/n.  All channels of the range must share one bandwidth B;
 * out: [count][B] complex64. */
int rcfm_tuner_run(rcfm_tuner_t t, int first, int count, void* out, void* stream);
/* Device pointer of the stored spectrum X [n] complex64 (Tuner._buffer). */
int rcfm_tuner_spectrum(rcfm_tuner_t t, void** X);
/* ---- the spectrum as an object that can travel (multi-GPU: rotating FFT owner, radiocore/tools/sharding.py) ------
 * Tuner.load (tuner.py:126-138) keeps the spectrum in `self._buffer`; with channels sharded over G GPUs only ONE GPU
 * needs to run the wideband FFT of a given buffer, if it then hands every peer the bins that peer's channels read.
 *   spectrum_layout   storage = [halo | n bins | halo] complex64 (the halos repeat the far ends: storage[0, halo) holds
 *                     bins [n - halo, n), storage[halo + n, halo + n + halo) bins [0, halo)); halo <= n / 2 always, and
 *                     halo = 0 -- no halos -- for a handle with a channel so wide that B / 2 + 2 bins, rounded up to
 *                     whole 128-byte lines, exceed n / 2
 *   attach_spectrum   use caller-owned storage of that layout instead of the handle's own (NULL: back to its own);
 *                     loaded_count > 0 declares that it already holds the bins of channels [loaded_first, +count)
 *   window            the bins channels [first, first + count) read: [first_bin, first_bin + nbins) modulo n, whole
 *                     rows of the forward plan (nbins = n: no window, everything)
 *   adopt             the caller has written those bins into the storage (received them over xGMI): refresh the
 *                     halos and accept exactly that channel range in rcfm_tuner_run / rcfm_pipeline_run
 *   window_layout     a rank that never OWNS a given buffer needs room for its window only: storage =
 *                     [halo | nbins | halo] complex64, the window's first bin at element `halo` (at G = 8 an eighth of
 *                     a spectrum per slot instead of a whole one).  RCFM_ERR_SIZE when the window wraps around bin 0
 *                     or touches the far ends (their halos repeat the other end): such a rank keeps whole slots
 *   attach_window     use such a storage for channels [first, first + count): receive the window's bins into
 *                     elements [halo, halo + nbins), then adopt(first, count).  rcfm_tuner_load and
 *                     rcfm_tuner_spectrum fail with RCFM_ERR_STATE while a window is attached; channels outside
 *                     the range are refused.  attach_spectrum (storage or NULL) ends it.                          */
int rcfm_tuner_spectrum_layout(rcfm_tuner_t t, int64_t* halo, int64_t* n);
int rcfm_tuner_attach_spectrum(rcfm_tuner_t t, void* storage, int loaded_first, int loaded_count);
int rcfm_tuner_window(rcfm_tuner_t t, int first, int count, int64_t* first_bin, int64_t* nbins);
int rcfm_tuner_window_layout(rcfm_tuner_t t, int first, int count, int64_t* halo, int64_t* nbins);
int rcfm_tuner_attach_window(rcfm_tuner_t t, void* storage, int first, int count);
int rcfm_tuner_adopt(rcfm_tuner_t t, int first, int count, void* stream);
/* ---- signal levels and squelch (no reference counterpart) ---------------------------------------------------------
 * The level of channel c (roll r, bandwidth B <= n) of the loaded spectrum X is the mean power of the samples
 * rcfm_tuner_run would return for it, taken from the B bins the channel reads, without the inverse FFT (Parseval):
 *   Y = the channel's length-B spectrum: bins k = 0 .. B/2 and their mirror images, each X[(k - r) mod n] times the
 *       fftshifted periodic Hann weight; for even B < n (B > 2) the two end bins +-B/2 ADDED before squaring;
 *   level[c] = sum_k |Y[k]|^2 / n^2 = mean(|rcfm_tuner_run(c)|^2): linear power in the units of the input samples.
 * The channels of a range may differ in bandwidth.  Readiness as for rcfm_tuner_run: RCFM_ERR_STATE before a load and
 * for a channel outside the range that was loaded, sharded or attached as a window, RCFM_ERR_INDEX for a bad range.
 * The sums have a fixed order: bit-identical from run to run and from stream to stream.
 * level[i] of channels [first, first+count), any mix of bandwidths; power: [count] float32 device */
int rcfm_tuner_levels(rcfm_tuner_t t, int first, int count, void* power, void* stream);
/* Squelch, per buffer and stateless (no hysteresis, no hang time): channel i is OPEN iff power[i] >= threshold[i]
 * (false when either is NaN); threshold: [count] float32 device, in the units of rcfm_tuner_levels.
 * open[i] = power[i] >= threshold[i]; rows of closed channels of audio [count][floats_per_channel] := 0.
 * audio may be NULL (mask only); open ([count] uint8 device) may be NULL.
 * Rows of open channels are neither read nor written.  Queue it behind rcfm_pipeline_run on the same stream: the
 * demodulators have then run on every channel, so the de-emphasis state of MFM / WBFM advances exactly as without
 * squelch and a channel that reopens carries the audio it would have carried anyway. */
int rcfm_squelch(const void* power, const void* threshold, int count, size_t floats_per_channel,
                 void* audio, void* open, void* stream);
/* ---- wideband power spectrum (no reference counterpart) ------------------------------------------------------------
 * What the band looks like between and around the channels: binned power and peak of the loaded spectrum X (unnormalised,
 * n bins).  A signed bin s in [-floor(n/2), n - floor(n/2)) means X[s mod n]; ascending s is ascending frequency, the
 * order numpy.fft.fftshift gives, and with one-second buffers s is Hz from the input frequency.  A span [s0, s0 + L),
 * L >= 1, lies inside that interval (it never wraps in frequency) and is cut into M cells, 1 <= M <= L: cell m covers
 * span positions e in [floor(m L / M), floor((m + 1) L / M)) (products in 64-bit integers), so cells differ in length
 * by at most one bin and none is empty.
 *   power[m] = sum over the cell of |X[(s0 + e) mod n]|^2 / n^2      float32
 *   peak[m]  = max over the cell of |X[(s0 + e) mod n]|^2 / n^2      float32
 * Linear power in the units of the input samples, the unit of rcfm_tuner_levels; over the full span the cells' power
 * adds up to mean(|x|^2) (Parseval).  peak keeps a narrow carrier visible in a wide cell.  Each |X|^2 is formed in float64
 * from the float32 re and im, summed in float64, scaled by 1 / n^2 in float64 and rounded to float32 once.
 * RCFM_ERR_ARG (checked before any device call): NULL handle, both outputs NULL, L < 1, M < 1, M > L, a span outside the
 * signed interval.  RCFM_ERR_STATE: before a load, or when a bin of the span is not held -- after a plain load (also into
 * an attached spectrum) every bin is; after a sharded load, an adopt or with a window attached, the bins of
 * rcfm_tuner_window for the range in force, containment taken modulo n.
 * The order of every sum depends on (n, s0, L, M) alone and there are no floating-point atomics: bit-identical from run
 * to run, from stream to stream, and whether one output is NULL or both are present.
 * first_bin = s0, nbins = L, cells = M; power, peak: [M] float32 device, either may be NULL */
int rcfm_tuner_power_spectrum(rcfm_tuner_t t, int64_t first_bin, int64_t nbins, int64_t cells, void* power, void* peak,
                              void* stream);
/* ---- carrier estimates and live retune (no reference counterpart) ----------------------------------------------------
 * Where inside its channel a station sits.  For channel c (roll r, bandwidth B <= n) of the loaded spectrum X the channel's
 * bins are the B signed offsets d = -floor(B/2) .. -floor(B/2) + B - 1 from the channel centre, bin d being element
 * X[(d - r) mod n] -- the indexing of rcfm_tuner_levels; with one-second buffers d is Hz above the channel's centre
 * frequency.  p_d = re^2 + im^2 of that element, formed in float64 from the float32 parts: no window weight and no Nyquist
 * merge (a carrier finder must not depend on the gather form, and the Hann taper over n is flat across a channel).
 *   peak_bin[i]   int32    the d of the largest p_d; on equal p_d the lowest d wins; a NaN p_d never wins
 *   peak_power[i] float32  that p_d / n^2, scaled in float64 and rounded once: the units of rcfm_tuner_levels and
 *                          rcfm_tuner_power_spectrum
 *   centroid[i]   float32  S1 / S0
 *   spread[i]     float32  sqrt(max(S2 / S0 - (S1 / S0)^2, 0))
 * with S_k = sum of d^k p_d over the gated-in bins: bin d is gated in iff p_d >= G, G = (double)gate n n computed once on
 * the host.  gate is power per bin in the units above, finite and >= 0; 0 takes every bin.  An ungated centroid of a weak
 * station is pulled to 0 by the channel's noise; a host derives the gate from the floor density it already computes.
 * When no bin is gated in (or S0 = 0) centroid = spread = 0.  The peak ignores the gate.
 * Each output is [count] on the device and may be NULL, but not all four.  The channels of a range may differ in
 * bandwidth.  Readiness as for rcfm_tuner_levels: RCFM_ERR_STATE before a load and for a channel outside the range that
 * was loaded, sharded or attached as a window, RCFM_ERR_INDEX for a bad range.  RCFM_ERR_ARG (checked before any device
 * call): NULL handle, all four outputs NULL, a negative or non-finite gate.
 * Every sum has one order, a function of B alone, and there are no floating-point atomics: bit-identical from run to
 * run, from stream to stream, and whichever outputs are NULL. */
int rcfm_tuner_carriers(rcfm_tuner_t t, int first, int count, float gate, void* peak_bin, void* peak_power, void* centroid,
                        void* spread, void* stream);
/* New rolls for channels [first, first + count): roll_host[i] replaces the roll of channel first + i, reduced modulo n as
 * rcfm_tuner_create reduces it.  Bandwidths, n, the halo, plans and storage stay as they are.  The host values are staged
 * before the call returns (the caller's array may be freed at once) and the device tables are updated in order on
 * `stream`: calls queued on that stream afterwards -- rcfm_tuner_run, rcfm_pipeline_run on every route, rcfm_tuner_levels,
 * rcfm_tuner_carriers -- see the new rolls.  The host must not have calls of this handle in flight on OTHER streams.
 * After a plain load every bin is held: the handle stays loaded and the same buffer can be run again at once.  Where the
 * storage holds a window only (a sharded load, rcfm_tuner_adopt, rcfm_tuner_attach_spectrum with loaded channels) the held
 * bins were chosen for the old rolls: the handle becomes not-loaded and reads return RCFM_ERR_STATE until the next
 * rcfm_tuner_load or rcfm_tuner_adopt; a declared shard (rcfm_tuner_shard) follows the new rolls from that load on.
 * RCFM_ERR_STATE while a window storage is attached (rcfm_tuner_attach_window): its layout was computed from the old
 * rolls.  RCFM_ERR_INDEX for a bad range, RCFM_ERR_ARG for a NULL handle or NULL rolls with count > 0. */
int rcfm_tuner_retune(rcfm_tuner_t t, int first, int count, const int64_t* roll_host, void* stream);
/* ---- IQ balance: imbalance estimate and image rejection on the loaded spectrum (no reference counterpart) ------------
 * A receiver whose I and Q paths differ in gain and phase delivers x' = mu x + nu conj(x): a station at +f puts an image of
 * itself at -f (5 % gain and 3 degrees phase error: 29 dB down).  In the loaded spectrum X (n bins) that reads
 * X'[k] = mu X[k] + nu conj(X[k']), with k' = (n - k) mod n the mirror of bin k.  Bin 0 is its own mirror; for even n, bin
 * n/2 is too.  With beta = nu / conj(mu), Y[k] = X'[k] - beta conj(X'[k']) = (mu - |nu|^2 / conj(mu)) X[k] exactly.
 *
 * Estimate.  Over the mirror pairs m in [m_lo, m_hi], 1 <= m_lo <= m_hi <= floor((n - 1) / 2) -- the self-mirrored bins are
 * never part of it, so a DC offset cannot bias it, and a host may calibrate on a region it trusts --
 *   P    = sum_m X[m] X[n - m]                      (complex product, no conjugate)
 *   Q    = sum_m (|X[m]|^2 + |X[n - m]|^2)
 *   c    = 2 P / Q
 *   beta = c / (1 + sqrt(1 - min(|c|^2, 1)))        (the exact inverse of c = 2 beta / (1 + |beta|^2))
 * Every product and square is formed in float64 from the float32 parts and summed in float64 in a fixed order that depends
 * on (n, m_lo, m_hi) alone; there are no floating-point atomics: bit-identical from run to run, from stream to stream, and
 * whether one output is NULL or both are present.  The finish computes beta in float64 and rounds once to float32; Q = 0 or
 * anything non-finite gives beta = 0.
 *   sums: [3] float64 device = Re P, Im P, Q; beta: [2] float32 device; either may be NULL, not both.
 * The estimate is blind: it takes what correlates between mirror bins for imbalance.  Two unmodulated carriers at exactly
 * mirrored frequencies correlate too and corrupt a per-buffer estimate; the answer is a range without them, or a fixed beta.
 * One beta for the whole band is a frequency-flat model of the receiver.
 *
 * Correct.  For every bin k, Y[k] = X[k] - beta conj(X[k']) in float32, beta [2] float32 read from DEVICE memory (what an
 * estimate on the same stream has just written, for instance); the self-mirrored bins use themselves.  Then, for a notch
 * half-width dc_notch = w >= 0, the bins of signed index |s| <= w - 1 are set to exact zero (w = 0: none; w = 1: bin 0, where
 * the receiver's DC offset sits).  Y replaces X in the storage, both halos included (spectrum_layout above): every later
 * rcfm_tuner_run, rcfm_pipeline_run, rcfm_tuner_levels, rcfm_tuner_power_spectrum, rcfm_tuner_carriers and
 * rcfm_pipeline_subcarrier reads the clean band.  A handle without halos works too.
 *
 * set_iq_balance.  RCFM_IQ_BALANCE_OFF (the default): a load launches what it launched before.  _FIXED: every
 * rcfm_tuner_load and rcfm_tuner_load_raw queues the correction with (beta_re, beta_im), kept in a device slot of the
 * handle, and the notch behind its FFT on the load's stream.  _AUTO: the estimate over all pairs, its finish and the
 * correction with that buffer's own beta (beta_re, beta_im are ignored).  No host synchronisation in either; nothing is
 * carried from buffer to buffer.  The host must not have loads of this handle in flight while it changes the setting.
 *
 * Readiness of estimate and correct as rcfm_tuner_power_spectrum over the full span: RCFM_ERR_STATE before a load and
 * whenever not every bin is held -- a sharded load, rcfm_tuner_adopt, an attached window; a plain load into the handle's own
 * spectrum or into an attached one is fine.  A load of a handle with a balance mode set whose shard keeps a window only
 * returns RCFM_ERR_STATE itself, before anything is launched.
 * RCFM_ERR_ARG, checked before any device call: NULL handle, both outputs NULL, NULL beta, an empty or out-of-range
 * [m_lo, m_hi] (this includes every n < 3, also for _AUTO), dc_notch negative or above n / 2, an unknown mode, a fixed
 * beta that is not finite or has |beta| >= 1. */
enum { RCFM_IQ_BALANCE_OFF = 0, RCFM_IQ_BALANCE_FIXED = 1, RCFM_IQ_BALANCE_AUTO = 2 };
int rcfm_tuner_iq_estimate(rcfm_tuner_t t, int64_t m_lo, int64_t m_hi, void* sums, void* beta, void* stream);
int rcfm_tuner_iq_correct(rcfm_tuner_t t, const void* beta, int64_t dc_notch, void* stream);
int rcfm_tuner_set_iq_balance(rcfm_tuner_t t, int mode, float beta_re, float beta_im, int64_t dc_notch);
int rcfm_tuner_destroy(rcfm_tuner_t t);

/* ---- demodulators (radiocore/analog/{fm,mfm,wbfm}.py) --------------------- */

/* C independent channels (or C consecutive buffers of distinct channels) of
 * identical geometry B -> A.  tau = deemphasis rate (mfm.py:32, wbfm.py:35).
 * chunk = channels processed per pass through the kernel chain (0 = default: 1024 at B = 240 000, proportionally
 * more for narrower channels up to 8192, i.e. the same workspace): bounds the workspace (about 9.6 MB per channel of
 * a 240 kHz WBFM chunk). */
int rcfm_demod_create(int kind, int C, int B, int A, double tau, int chunk, rcfm_demod_t* out);
/* FM.run / MFM.run / WBFM.run on channels [first, first+count):
 * iq [count][B] complex64 -> audio [count][A][ch] float32. */
int rcfm_demod_run(rcfm_demod_t d, int first, int count, const void* iq, void* audio,
                   void* stream);
/* De-emphasis filter state, the reference's Deemphasis._state (deemphasis.py:48-49,64):
 * [C][ch][50] float32, host memory.  reset = lfilter_zi(taps) for every channel. */
int rcfm_demod_reset_state(rcfm_demod_t d, void* stream);
int rcfm_demod_get_state(rcfm_demod_t d, float* state_host, void* stream);
int rcfm_demod_set_state(rcfm_demod_t d, const float* state_host, void* stream);
/* Design outputs for parity checks: 51 de-emphasis taps, 41 pilot band-pass taps
 * (host, float32).  Either pointer may be NULL. */
int rcfm_demod_get_taps(rcfm_demod_t d, float* deemph51_host, float* pilot41_host);
/* One de-emphasis state per channel, whoever runs it: makes the one-channel handle `single` (the demodulator object
 * a Channel carries, tuner.py:24) keep its state in slot `index` of `batched` (the handle rcfm_pipeline_run uses for
 * all channels) from now on; move_history != 0: what `single` has carried so far is moved into the slot (it has run
 * before), 0: the slot's content stands (`single` is new, the batched handle has the history).  Afterwards a caller may mix
 * `demodulator.run(tuner.run(i))` (multi_fm_server.py:101-102) and the batched call across buffers and get the
 * reference's results: there, the state lives in the demodulator object (deemphasis.py:48-49,64) and nowhere else.
 * `single` may itself hold several channels (slots [index, index + its C) are taken: two batched handles of one
 * geometry then share one state).  Same class, audio rate and time constant required; FM has no state (no-op). */
int rcfm_demod_bind_state(rcfm_demod_t single, rcfm_demod_t batched, int index, int move_history, void* stream);
/* Per-handle options a HOST may need (the kernel-form switches that tools and tests use live in rcfm_tools.h).
 *   RCFM_OPT_NARROW_TILES the tile kernels exist with 16 and with 8 lines per tile: 0 = always 16, 1 (default) = 8 when a
 *                         launch has fewer than two 16-line tiles per CU (one WBFM.run per call, the reference's harness
 *                         shape tests/benchmark.py:29-31: 60 short tiles instead of 30 long ones), 2 = always 8; applies
 *                         to the demodulator's kernels and, in rcfm_pipeline_run, to the tuner's inverse FFT of the chunk
 *   RCFM_OPT_STATE_FENCE  (default 0) consecutive buffers on DIFFERENT streams: the reference's loop
 *                         (examples/multi_fm_server.py:98-106) handles one buffer at a time; a host that keeps two handle
 *                         sets (tuner + demodulator, the second demodulator bound to the first one's state with
 *                         rcfm_demod_bind_state) and alternates them, each on its own stream, lets the kernels of buffer
 *                         i + 1 fill the gaps of buffer i.  The de-emphasis state is the one thing buffer i + 1 needs
 *                         from buffer i (deemphasis.py:64): with the fence on, every launch sequence that touches the
 *                         shared state waits for the event the previous one recorded, on whichever stream that was.
 *                         Set it on any ONE handle of the sharing group, after the binding
 *   RCFM_OPT_GRAPH        (default 0) a handle of ONE channel (the reference's per-channel call, fm.py:46 / mfm.py:51 /
 *                         wbfm.py:66; tests/benchmark.py:29-31 times exactly these) replays its launch chain from a
 *                         captured hipGraph when the call's pointers and stream kind repeat: one graph launch instead of
 *                         ten kernel launches.  0: plain launches.  Results are bit-identical either way.  Off by default: on ROCm 7 the
 *                         graph launch costs as much as the launches it replaces (profiles/r06_a_single_call.txt) */
enum { RCFM_OPT_NARROW_TILES = 4, RCFM_OPT_STATE_FENCE = 5, RCFM_OPT_GRAPH = 10 };
int rcfm_demod_set_option(rcfm_demod_t d, int option, int value);
int rcfm_demod_destroy(rcfm_demod_t d);

/* ---- stateful AGC for AM and SSB (no reference counterpart) ----------------------------------------------------------
 * RCFM_AM, RCFM_USB and RCFM_LSB normalise every buffer by a statistic of that buffer alone (the carrier mean, the RMS):
 * the gain steps at every buffer boundary, and a speaker who pauses comes out louder in that buffer than in its neighbours.
 * An AGC replaces that statistic by a follower whose value is carried from buffer to buffer.
 *
 * Definition.  A row is v[0..n), float32, at audio rate.  Parameters: decay_samples > 0, with
 * lambda = exp(-1 / decay_samples) and alpha = 1 - lambda (both formed in float64); level > 0; floor >= 0; all finite; and
 * one float32 of state s per row.
 *   RCFM_AGC_PEAK (USB / LSB)   e[n] = max(|v[n]|, lambda e[n-1]),           e[-1] = s
 *                               audio[n] = clip(level v[n] / max(e[n], floor), +-0.999)
 *   RCFM_AGC_CARRIER (AM)       c[n] = c[n-1] + alpha (v[n] - c[n-1]),       c[-1] = s
 *                               audio[n] = clip(level (v[n] - c[n]) / max(c[n], floor), +-0.999)
 * In both modes the output is 0 where the denominator is not > 0, and s becomes the follower's value after the last
 * sample.  s < 0 (the reset value -1) means "no history": PEAK starts from e[-1] = 0, CARRIER from c[-1] = mean(v) of this
 * call's row, summed in float64 in a fixed order.  floor bounds the gain at level / floor, so an empty channel does not
 * come out at full scale.  Non-finite input may spoil its own row from that sample on, never another row.
 * Evaluation.  PEAK never multiplies lambda in sample after sample: e[n] is the largest |v[k]| exp2(-(n - k) log2(e) /
 * decay_samples), evaluated from that sample, the exponent in float64.  CARRIER runs its recurrence in float64 in the
 * c + alpha (v - c) form, whose DC gain is exactly 1.  There are no atomics and the order of every operation is a function
 * of n alone: bit-identical from run to run, from stream to stream, for a sub-range of rows against the whole range and
 * for any chunk of a demodulator.
 *
 * rcfm_agc        the primitive: v [C][n] -> audio [C][n], state [C] float32 DEVICE, read and updated.  audio == v (in
 *                 place) is allowed, any other overlap is refused.  C within the primitives' limit below.
 *                 RCFM_ERR_ARG, before any device call: a NULL pointer, C < 1 or > 65535, n < 1, an unknown mode,
 *                 decay_samples not finite or <= 0, level not finite or <= 0, floor not finite or < 0, partial overlap.
 * set_agc         AM handles select CARRIER, USB / LSB handles PEAK; any other kind: RCFM_ERR_ARG.  decay_samples == 0
 *                 switches the AGC off again (the default; level and floor are then ignored).  With AGC on, the handle
 *                 runs the AGC tail in place of its per-buffer normalisation on every route of rcfm_demod_run and
 *                 rcfm_pipeline_run.  The handle owns one state float per channel; set_agc (on) gives the handle a fresh
 *                 state of its own, reset to -1, so call it before rcfm_demod_bind_state.
 *                 rcfm_demod_reset_state resets the AGC state to -1 as well.
 * get / set_agc_state   [C] float32, host memory; RCFM_ERR_STATE while the AGC is off.
 * rcfm_demod_bind_state shares the AGC state the way it shares the de-emphasis state (slot `index` of `batched`), and
 *                 requires equal AGC settings on both handles; RCFM_OPT_STATE_FENCE orders the AGC tail across streams.
 * RCFM_OPT_GRAPH  a handle with AGC on does not capture: it keeps launching its chain, whatever the option says.
 * Profile stages  the AGC tail is timed as the stage of the kernel it replaces (am_tail, ssb_tail). */
enum { RCFM_AGC_PEAK = 0, RCFM_AGC_CARRIER = 1 };
int rcfm_demod_set_agc(rcfm_demod_t d, double decay_samples, float level, float floor);
int rcfm_demod_get_agc_state(rcfm_demod_t d, float* state_host, void* stream);
int rcfm_demod_set_agc_state(rcfm_demod_t d, const float* state_host, void* stream);

/* Whole hot path for one wideband buffer already loaded with rcfm_tuner_load:
 * the loop of examples/multi_fm_server.py:100-106 (run -> demodulator.run) for
 * channels [first, first+count), chunk by chunk.  audio: [count][A][ch]. */
int rcfm_pipeline_run(rcfm_tuner_t t, rcfm_demod_t d, int first, int count, void* audio,
                      void* stream);

/* ---- subcarrier tap (no reference counterpart) ------------------------------------------------------------------------
 * What else the FM multiplex carries: RDS at 57 kHz, SCA at 67 / 92 kHz, DARC at 76 kHz, the CTCSS tone of narrow FM.  For
 * every channel of a range, the complex baseband of the multiplex around a subcarrier frequency f, low-pass filtered and
 * decimated to a rate a host can handle; phase loop, bit timing and decoding stay on the host (radiocore.tools.rds).
 *
 * Inputs.  For the B channel samples x[0..B) of one channel (one-second buffers, so B is also the sample rate in Hz):
 *   f        an integer subcarrier frequency in Hz, |f| <= B/2;
 *   R        an output length that divides B, with D = B / R;
 *   h[0..T)  T real taps, T odd, 1 <= T <= 4095, centre c = (T-1)/2.
 * Discriminator (the FM discriminator of fm.py:60-65).
 *   th[n] = arg(x[n]) / pi
 *   d[0]  = 0
 *   d[n]  = th[n] - th[n-1], wrapped into [-1, 1]
 *   d[n]  = 0 outside [0, B)
 * Output, complex64 [count][R].
 *   y[j]  = sum_{i=0}^{T-1} h[i] d[jD + i - c] exp(-2 pi i ((jD + i - c) f mod B) / B),   j = 0 .. R-1
 * In words: mix the multiplex down by f, low-pass with h, keep every D-th sample.  Edges are a linear convolution with zero
 * extension, not circular.  A subcarrier at f with frequency deviation Delta Hz and phase phi comes out as
 * (Delta / B) sum(h) e^{i phi}.  The phase index (n f) mod B is exact integer arithmetic in 64 bits: at B = 240 000,
 * f = 57 000 the product passes 2^32.
 * Evaluation form.  The library evaluates
 *   y[j]   = rot[j] sum_i g[i] d[jD + i - c]
 *   g[i]   = h[i] exp(-2 pi i ((i-c) f mod B) / B)
 *   rot[j] = exp(-2 pi i (jD f mod B) / B)
 * with g and rot computed on the host in float64 and stored as complex64 tables.
 * Determinism.  Every output's sum over i has one order, the same for every output of a handle: taps i = p, p + D, p + 2D, ...
 * for p = 0, 1, .. in turn, a function of T and D alone (where no tile of the kernel fits the LDS, D of several thousand:
 * 256 interleaved partial sums folded in a fixed tree, a function of T alone).  There are no floating-point atomics.  Results
 * are bit-identical from run to run, from stream to stream, for a sub-range against the whole range, and for any chunk.
 *
 * create   RCFM_ERR_ARG before any device call for NULL pointers, C < 1, B < 2, R < 1, B % R != 0, |f| > B/2, ntaps even or
 *          outside 1 .. 4095, a non-finite tap.  C = the most channels one call will pass; chunk as for rcfm_demod_create
 *          (0 = 1024 channels at B = 240 000, proportionally more for narrower channels, up to 8192).  The handle owns g and
 *          rot on the device and, for the pipeline form, one workspace of chunk B float32 (complex64 for a band whose inverse
 *          FFT cannot leave phases): plain device memory, never taken from a bound arena.
 * run      the from-samples form, as rcfm_demod_run is for the demodulators: iq [count][B] complex64 -> out [count][R].
 * pipeline channels [first, first + count) of a loaded tuner, chunk by chunk: the tuner's inverse FFT leaves angle(x) / pi
 *          in the workspace where its band can (else the samples), and the tap kernel reads that.  Readiness as for
 *          rcfm_pipeline_run: RCFM_ERR_STATE before a load or outside the loaded / sharded / attached range, RCFM_ERR_INDEX
 *          for a bad range (or count > C), RCFM_ERR_SIZE where a channel's bandwidth is not B.  It touches no demodulator
 *          workspace or state. */
int rcfm_subcarrier_create(int C, int B, int R, int64_t f, const float* taps_host, int ntaps, int chunk, rcfm_subcarrier_t* out);
int rcfm_subcarrier_run(rcfm_subcarrier_t h, int count, const void* iq, void* out, void* stream);      /* iq [count][B] complex64 */
int rcfm_pipeline_subcarrier(rcfm_tuner_t t, rcfm_subcarrier_t h, int first, int count, void* out, void* stream);
int rcfm_subcarrier_destroy(rcfm_subcarrier_t h);

/* ---- audio egress: the open channels' audio, packed densely as PCM (no reference counterpart) -------------------------
 * Every route ends in audio [count][row] float32 on the device, row = A ch (the floats_per_channel of rcfm_squelch).  A
 * publisher wants 16-bit PCM of the channels that are open, and only those should cross PCIe.
 *
 * Definition.  open: [count] uint8 as rcfm_squelch writes it, any nonzero byte is open; NULL: every channel is open.
 *   slot(c)              = the number of open channels below c (channel order is kept)
 *   n_open               = the number of open channels
 *   index[slot(c)]       = c                        for every open channel c
 *   packed[slot(c)][i]   = q(audio[c][i])           for every open channel c, i = 0 .. row-1
 * The conversion q:
 *   RCFM_PCM_F32   the 32 bits unchanged (NaN payloads survive); gain is ignored
 *   RCFM_PCM_S16   y = x * gain, one float32 multiply; NaN -> 0; otherwise round to nearest, ties to even, then clamp to
 *                  [-32767, 32767]: the range is symmetric (-32768 never appears), +-inf and products that overflow
 *                  saturate.  gain is finite and in (0, 2^24]: below that bound a float32 denormal times gain rounds to 0
 *                  whether or not denormals are flushed, so the result does not depend on the denormal mode.
 * audio: [count][row] float32 device; packed: [count][row] int16 or float32 device, the worst-case capacity; index:
 * [count] int32 device; n_open: one int32 device.  index and n_open may be NULL, packed may not.  Rows of closed channels
 * are not read.  Rows >= n_open of packed and entries >= n_open of index are not written.
 * There are no atomics and every output is a function of the inputs alone: bit-identical from run to run and from stream
 * to stream.  (The slots come from one scan of the mask into a table the library keeps per stream; the pack reads it.)
 * RCFM_ERR_ARG, checked before any device call: NULL audio or packed, count < 1 or > 65535, row < 1, an unknown format, a
 * gain that is not finite or outside (0, 2^24] (RCFM_PCM_S16 only), any overlap of audio [count][row] with packed
 * [count][row], a pointer not aligned for one element of its type. */
enum { RCFM_PCM_F32 = 0, RCFM_PCM_S16 = 1 };
int rcfm_audio_pack(const void* audio, const void* open, int count, size_t row, int format, float gain,
                    void* packed, void* index, void* n_open, void* stream);

/* ---- tone bank: CTCSS / SELCAL detection and tone squelch on the audio (no reference counterpart) -------------------------
 * The signalling tones a receiver of these bands is expected to understand: the CTCSS tone (67 .. 254 Hz) that separates the
 * users of one narrow-FM channel, the two tone pairs of an aeronautical SELCAL call.  After rcfm_pipeline_run the audio
 * [C][A][ch] lies on the device; the tone bank gives, per channel and time frame, the power at each of K given frequencies
 * and the frame's total power, for FM, AM and SSB audio alike.
 *
 * Definition.  One channel's audio is x[0..A), float32, read from audio[c][i step + offset] with step in {1, 2} and
 * 0 <= offset < step (a row holds A step floats: step = 2 addresses one side of WBFM's interleaved stereo).  A bank has
 *   K        tones, 1 <= K <= 64;
 *   nu[k]    double, cycles per sample, finite, 0 <= nu[k] <= 0.5;
 *   L        a frame length, 1 <= L (this library: L <= 2^24, so that the coarse table below, K ceil(L / 16) complex64 built
 *            on the host, stays below 512 MiB; the definition has no upper limit and nothing else depends on this one);
 *   w[0..L)  an optional real window, float32, every element finite, S = sum w[i] (taken in float64) > 0; NULL: w = 1.
 * F = floor(A / L) frames; a tail of A mod L samples is not read; A < L is RCFM_ERR_SIZE at run.
 *   Z[c][f][k] = (1/S) sum_{i=0}^{L-1} w[i] x_c[f L + i] exp(-2 pi j frac(nu[k] i))      (the phase is frame-local)
 *   P[c][f][k] = |Z[c][f][k]|^2               float32 [count][F][K]
 *   E[c][f]    = (1/L) sum_i x_c[f L + i]^2   float32 [count][F]     (no window)
 * A sinusoid of amplitude a exactly at nu[k] gives P ~ a^2 / 4 for any window; P / E is the share of the frame's power at
 * the tone, and detection is thresholded on that ratio.
 * Evaluation form.  exp(-2 pi j frac(nu (16 m + j))) = coarse[k][m] fine[k][j], j = 0 .. 15: both tables are computed on the
 * host with frac(nu i) in float64 and stored as complex64; per 16 samples and tone the device forms
 * sum_j (x w)[16 m + j] fine[k][j] with float32 FMAs and multiplies it by coarse[k][m].  No recurrence runs over a frame and
 * no sine or cosine is evaluated on the device.  |Z|^2 / S^2 is formed in float64 from the float32 sums and rounded once;
 * the energy is summed in float64 and rounded once.
 * Determinism.  No atomics.  Every sum has one order, a function of (L, K) alone: bit-identical from run to run, from stream
 * to stream, for a sub-range of channels against the whole range, and whether energy is NULL or not.  (A frame longer than
 * 8192 samples is split over ceil(L / 8192) workgroups whose float sums a finish step adds in segment order; they pass
 * through a buffer the handle keeps per stream.)
 * Such a bank (L > 8192 only) is asynchronous from its second run on a stream on: the first run on a stream, and a later one
 * with more channels than any before it on that stream (up to 65 535 are sized for), allocates that buffer with hipMalloc --
 * growth frees the old one first, which waits for the device -- so do not make that run inside a stream capture; warm the
 * bank up with the largest count first.  The buffers, count F ceil(L / 8192) (8 K' + 8) bytes each with K' = K rounded up
 * to a multiple of 8, are kept per stream handle until rcfm_tone_bank_destroy: a host that keeps creating and destroying
 * streams should run its banks of long frames on streams it keeps.  Banks with L <= 8192 own no such buffer and never allocate
 * in run.
 *
 * create   nu_host [K], window_host [L] or NULL.  RCFM_ERR_ARG before any device call: a NULL pointer, K outside 1 .. 64,
 *          L outside 1 .. 2^24, a nu that is not finite or outside [0, 0.5], a window element that is not finite, S <= 0.
 * run      audio [count][A step] float32 -> power [count][F][K], energy [count][F] (may be NULL), asynchronously on `stream`.
 *          RCFM_ERR_ARG before any device call: a NULL handle, audio or power, count < 1, A < 1, step outside {1, 2}, offset
 *          outside [0, step), a pointer not aligned for a float.  RCFM_ERR_SIZE: A < L.
 *
 * Tone squelch.  rcfm_tone_score computes, for each channel c of power [count][F][K] and energy [count][F]:
 *   score[c] = max_f P[c][f][want[c]] / E[c][f]      frames with E == 0 contribute 0, a NaN ratio never wins
 *   want[c] == -1          score[c] = +inf: no tone is required
 *   gate[c] == 0           score[c] = NaN, whatever want[c] is (gate: [count] uint8, the open mask of a level squelch, or NULL)
 * score then goes through rcfm_squelch(score, ratio_threshold, ...), which opens on score >= threshold and is false for NaN:
 * the zero fill, the open mask, rcfm_audio_pack and the drain work unchanged, and a level squelch and a tone squelch combine
 * through gate.  want is an int32 [count] DEVICE array, so it cannot be validated before the launch: a host checks its range
 * (radiocore's Tuner.set_tones does), and the kernel defines the rest -- a want[c] outside [-1, K) reads no memory and gives
 * NaN, a channel that never opens.
 *          RCFM_ERR_ARG before any device call: NULL power, energy, want or score, count < 1, F < 1, K outside 1 .. 64, a
 *          pointer not aligned for its element. */
int rcfm_tone_bank_create(int K, const double* nu_host, int L, const float* window_host, rcfm_tone_bank_t* out);
int rcfm_tone_bank_run(rcfm_tone_bank_t b, const void* audio, int count, int A, int step, int offset, void* power, void* energy,
                       void* stream);
int rcfm_tone_bank_destroy(rcfm_tone_bank_t b);
int rcfm_tone_score(const void* power, const void* energy, const void* want, const void* gate, int count, int F, int K,
                    void* score, void* stream);

/* ---- audio filter: biquad sections per channel, carried across buffers (no reference counterpart) -------------------------
 * What a receiver applies to a narrow-band channel's audio before its speaker: the 300 Hz high-pass that strips the CTCSS
 * tone, narrow FM's de-emphasis, the voice band-pass of an airband set.  Such filters are recursive: a few second-order
 * sections where an FIR of the same slope needs hundreds to thousands of taps.
 *
 * Definition.  A filter is S sections, 1 <= S <= 8; section s is b0 b1 b2 a0 a1 a2 in float64, the row layout of scipy's
 * `sos`.  a0 must be exactly 1, every coefficient finite, every section strictly stable: |a2| < 1 and |a1| < 1 + a2.
 * One row is x[0..n), float32.  Section s maps its input u to its output y in transposed direct form II, the form of
 * scipy.signal.sosfilt:
 *   y[i] = b0 u[i] + z0
 *   z0'  = b1 u[i] - a1 y[i] + z1
 *   z1'  = b2 u[i] - a2 y[i]
 * Section s + 1 reads section s's output; the last section's output is rounded once to float32.  All of the recurrence's
 * arithmetic -- runs, aggregates, scan, carries, state -- is float64: a float32 recurrence is off by 1e-5 .. 6e-5 of the
 * row's peak for the voice filters at 48 kHz, this form by 5e-8.
 * State.  (z0, z1) per channel, per leg and per section, float64 [C][ch][S][2], carried from call to call: filtering a row
 * of 2 n samples equals two calls of n, up to rounding.  It is all zeros after create and after reset: these are sosfilt's
 * zero initial conditions (a filter at rest), NOT scipy.signal.sosfilt_zi's steady state of a step -- a row with a DC level
 * starts with the filter's step response.  The library does not inspect the data: a NaN or infinity in a row stays in that
 * row's state until a reset.
 * Layout.  The audio is [count][n][ch], ch in {1, 2}; with ch = 2 the row is WBFM's interleaved stereo, and each leg is a
 * row of its own with its own state.
 * Evaluation form.  One workgroup per channel; the row passes through on-chip memory in segments of 8192 floats, read once
 * and written once whatever S is.  Thread t owns a run of R = 33 samples.  Per section: the recurrence over the run from
 * zero state gives the run's end state v_t; the state entering run t follows s_t = M^R s_(t-1) + v_(t-1) with
 * M = [[-a1, 1], [-a2, 0]], an affine scan with host-built float64 tables M^(R 2^k), k = 0 .. 5, and M^(64 R); the run is
 * then repeated from s_t.  The tables only decay, since sections are stable.
 * Determinism.  No atomics; the order of every operation is a function of (n, ch, S) alone: bit-identical from run to run,
 * from stream to stream, for a sub-range of channels against the whole range, in place against out of place, whatever the
 * alignment of the rows, and with select NULL against all ones.
 *
 * create     sos_host [S][6].  RCFM_ERR_ARG before any device call: a NULL pointer, C < 1, ch outside {1, 2}, S outside
 *            1 .. 8, a coefficient that is not finite, a0 != 1, an unstable section.  Everything a run needs is built here.
 * run        filters rows [0, count) of `in` into `out` with the state slots of channels first .. first + count - 1,
 *            asynchronously on `stream`, without a device allocation or a host synchronisation.  out == in is allowed; any
 *            other overlap is the caller's error.  select: uint8 [count] on the device, or NULL for all; a row with
 *            select[c] == 0 is copied unchanged (not touched at all in place) and its state does not advance.
 *            RCFM_ERR_ARG before any device call: a NULL handle, in or out, count < 1, n < 1, a pointer not aligned for a
 *            float.  RCFM_ERR_INDEX: first < 0 or first + count > C.
 * reset      all states back to zero, on `stream`.
 * get_state / set_state   the whole state, float64 [C][ch][S][2], to / from the host; both wait for `stream`.
 * set_fence  as RCFM_OPT_STATE_FENCE: when on, a run waits for the event the previous run of this handle recorded and
 *            records its own, so one handle may serve consecutive buffers on different streams.  Off by default, and then
 *            no event is touched. */
int rcfm_audio_filter_create(int C, int ch, int S, const double* sos_host, rcfm_audio_filter_t* out);
int rcfm_audio_filter_run(rcfm_audio_filter_t f, int first, int count, int n, const void* in, void* out, const void* select,
                          void* stream);
int rcfm_audio_filter_reset(rcfm_audio_filter_t f, void* stream);
int rcfm_audio_filter_get_state(rcfm_audio_filter_t f, double* state_host, void* stream);
int rcfm_audio_filter_set_state(rcfm_audio_filter_t f, const double* state_host, void* stream);
int rcfm_audio_filter_set_fence(rcfm_audio_filter_t f, int on);
int rcfm_audio_filter_destroy(rcfm_audio_filter_t f);

/* ---- frame gate: time-resolved squelch with hysteresis, hang time and look-ahead (no reference counterpart) --------------
 * rcfm_squelch decides once per buffer and keeps no memory.  The frame gate cuts the buffer into F frames, measures each
 * frame's power, and walks a per-channel state machine over them that is carried from buffer to buffer: a transmission
 * that starts inside a buffer opens from its first frame, a level near the threshold does not chatter, and a speaker's
 * pause does not close the channel.
 *
 * rcfm_frame_power.  x is [rows][n], float32 (is_complex = 0) or complex64 (is_complex != 0); power is [rows][F] float32,
 * F = floor(n / L): power[r][f] = (1 / L) sum_{i < L} |x[r][f L + i]|^2.  The tail n mod L is not read.  Squares and sums
 * are float64 on the float32 values, the result is divided by L and rounded once to float32.  A frame is m = L or 2 L
 * floats.  Up to 4096 floats it belongs to one wave (four frames to a workgroup, never a frame shared between waves); a
 * longer one is cut into segments of 16384 floats, one workgroup each, whose float64 sums a second kernel adds in segment
 * order (the partial sums live in a library-owned buffer per stream, grown by the first call that needs more).  Inside a
 * wave or workgroup the floats are taken in groups of four, group g by lane g mod 64 (thread g mod 256), element e of every
 * group into the lane's accumulator e, the lanes' sums in a fixed tree, the waves' sums in order.  No atomics; the order of
 * every sum is a function of (L, is_complex) alone: bit-identical from run to run, between streams, for a sub-range of rows
 * and whatever the rows' alignment -- the alignment of a frame's first float only picks the load, 16 bytes per lane, else
 * 8, else 4.  RCFM_ERR_ARG before any device call: a NULL pointer, rows < 0, L < 1, L > n, L > 2^30, x not aligned for its
 * element or power not for a float, rows F above 2^31 - 1.
 *
 * rcfm_tuner_frame_levels.  power [count][F] float32: the frame power of the samples rcfm_tuner_run returns for channels
 * first .. first + count - 1, frames of B / F samples.  Readiness and the shared-bandwidth rule are rcfm_tuner_run's
 * (RCFM_ERR_STATE, RCFM_ERR_INDEX, RCFM_ERR_ARG); F must divide B, else RCFM_ERR_ARG.  scratch is caller-owned device memory
 * for m = floor(scratch_bytes / (8 B)) >= 1 channels.  The call IS, chunk by chunk on `stream`,
 *   for (i = 0; i < count; i += m)  rcfm_tuner_run(t, first + i, min(m, count - i), scratch, stream);
 *                                   rcfm_frame_power(scratch, min(m, count - i), B, 1, B / F, power + i F, stream);
 * so it costs one more inverse pass of the channels plus 8 B bytes written and read per channel; the mean of a channel's
 * frames is rcfm_tuner_levels' value up to the rounding of the inverse FFT.
 *
 * The gate.  State: (open, hang_left) per channel, int32 [C][2], addressed by channel index; zero after create and reset.
 * create     hang: frames a channel stays open below close_thr; lead: frames of look-ahead; ramp_host [R] float32, the
 *            rising edge's gains (Tuner builds 0.5 - 0.5 cos(pi (i + 1) / (R + 1)) in float64, rounded once), R >= 0.
 *            RCFM_ERR_ARG before any device call: out NULL, C < 1, hang < 0, lead < 0, R outside 0 .. 2^20, R > 0 with
 *            ramp_host NULL, a ramp element that is not finite.
 * run        power [count][F], open_thr and close_thr [count] float32, frame_mask [count][F + 1] uint8, open_any [count]
 *            uint8 or NULL, all on the device and all indexed by row: row i is channel first + i, whose state slot it uses.
 *            One thread per channel walks the frames in order:
 *              column 0 of frame_mask is the state's `open` on entry (the previous buffer's last frame, undilated);
 *              for each frame with power p:  if p >= open_thr: open = 1, hang_left = hang;
 *                                            else if open and p >= close_thr: hang_left = hang;
 *                                            else if open: hang_left > 0 ? hang_left -= 1 : open = 0;
 *              comparisons with NaN are false; g[f] = open.
 *            Look-ahead: g'[f] = g[f] | g[f + 1] | ... | g[min(f + lead, F - 1)], so a transmission's onset is not clipped;
 *            frame_mask[c][f + 1] = g'[f]; open_any[c] = g'[0] | ... | g'[F - 1] | column 0 (a channel that closes exactly at
 *            the buffer edge still gets its ramp-down published).  The stored state is the undilated one.
 *            RCFM_ERR_ARG before any device call: a NULL handle, power, threshold or frame_mask, count < 0, F outside
 *            1 .. 65535, a pointer not aligned for a float.  RCFM_ERR_INDEX: first < 0 or first + count > C.
 * apply      audio [count][A][ch] float32, ch in {1, 2}, in place; F must divide A, La = A / F.  Frame f of row c, with
 *            g = frame_mask[c][f + 1] and gp = frame_mask[c][f], samples i < La, both legs alike:
 *              g = 1, gp = 1   neither read nor written
 *              g = 0, gp = 0   +0.0f stored
 *              g = 1, gp = 0   x r[i] for i < R, untouched from R on
 *              g = 0, gp = 1   x r[R - 1 - i] for i < R, +0.0f from R on
 *            The multiply is one float32 product.  16-byte stores where La ch is a multiple of 4 and audio is 16-byte
 *            aligned, else 4-byte stores.  It touches no state.  RCFM_ERR_ARG before any device call: a NULL handle, mask or
 *            audio, count < 0, F outside 1 .. 65535, A < 1, F not dividing A, ch outside {1, 2}, audio not aligned for a
 *            float, R > A / F.
 * run and apply are asynchronous on `stream`, without a device allocation or a host synchronisation.
 * reset      all states back to zero, on `stream`.
 * get_state / set_state   the whole state, int32 [C][2], to / from the host; both wait for `stream`.
 * set_fence  as rcfm_audio_filter_set_fence: when on, a run waits for the event the previous run of this handle recorded
 *            and records its own.  Off by default, and then no event is touched. */
int rcfm_frame_power(const void* x, int rows, int64_t n, int is_complex, int L, void* power, void* stream);
int rcfm_tuner_frame_levels(rcfm_tuner_t t, int first, int count, int F, void* scratch, size_t scratch_bytes, void* power,
                            void* stream);
int rcfm_gate_create(int C, int hang, int lead, const float* ramp_host, int R, rcfm_gate_t* out);
int rcfm_gate_run(rcfm_gate_t g, int first, int count, int F, const void* power, const void* open_thr, const void* close_thr,
                  void* frame_mask, void* open_any, void* stream);
int rcfm_gate_apply(rcfm_gate_t g, const void* frame_mask, int count, int F, int A, int ch, void* audio, void* stream);
int rcfm_gate_reset(rcfm_gate_t g, void* stream);
int rcfm_gate_get_state(rcfm_gate_t g, int32_t* state_host, void* stream);
int rcfm_gate_set_state(rcfm_gate_t g, const int32_t* state_host, void* stream);
int rcfm_gate_set_fence(rcfm_gate_t g, int on);
int rcfm_gate_destroy(rcfm_gate_t g);

/* ---- noise floor: OS-CFAR thresholds from the power spectrum, tracked across buffers (no reference counterpart) -----------
 * rcfm_squelch and the frame gate compare against absolute levels a host has to supply, and a band is not flat.  The noise
 * floor takes, around every cell of rcfm_tuner_power_spectrum's output, an order statistic of the neighbouring cells (guard
 * cells next to it left out, so a station does not raise its own floor), smooths it from buffer to buffer on the device and
 * turns it into per-channel thresholds on the device: "10 dB over the floor here and now", without a host round trip.
 *
 * Ordering.  Values are ordered by value; -0 sorts below +0; every NaN sorts above +inf, and all NaNs are equal.  A NaN
 * result is stored as 0x7fc00000.
 *
 * rcfm_rank_filter.  x, out: [M] float32 on the device, stateless.  The candidates of cell m are the cells j with
 * 0 <= j < M and guard < |j - m| <= half: no padding, no reflection, at the band ends the window is shorter.  With cnt
 * candidates, out[m] is the candidate of rank r = (q (cnt - 1)) / 1000 (64-bit integer division; 0-based, ascending in the
 * ordering above), the bits of that input cell.  q = 0 is the minimum, 500 the (lower) median, 1000 the maximum.  A cell
 * that has no candidate (possible for M < 2 guard + 2) gets NaN.  The selection is exact (a bisection over the 32 bits of
 * an order-preserving key, counting the candidates below the pivot), so the output bits do not depend on how it is computed:
 * the same from run to run, from stream to stream and for any alignment.  RCFM_ERR_ARG before any device call: a NULL
 * pointer, out == x, M < guard + 2, M > 2^30, half outside 1 .. 4096, guard outside 0 .. half - 1, q outside 0 .. 1000, a
 * pointer not aligned for a float.
 *
 * The handle.  State s [M] float32 on the device, all NaN ("not primed") after create and reset.
 * create     M, half, guard, q as above; rise, fall: the smoothing factors, finite and in (0, 1].  RCFM_ERR_ARG before any
 *            device call: out NULL, the refusals of rcfm_rank_filter, rise or fall outside (0, 1] or not finite.
 * run        power [M] float32 device (rcfm_tuner_power_spectrum's); e = rank_filter(power); then per cell
 *              s' = e                                     if s is NaN
 *              s' = s                                     if e is NaN
 *              s' = s + a (e - s), a = e > s ? rise : fall  else, as __fadd_rn(s, __fmul_rn(a, __fsub_rn(e, s))): three
 *                                                          float32 roundings, no contraction
 *            s' replaces s; floor [M] float32 = s'; over [M] uint8 = power[m] >= __fmul_rn(ratio, s'[m]) (false on NaN).
 *            floor or over may be NULL, not both.  One kernel, asynchronous on `stream`, no device allocation, no host
 *            synchronisation.  RCFM_ERR_ARG before any device call: a NULL handle or power, floor and over both NULL,
 *            floor == power, a NaN ratio, power or floor not aligned for a float.
 * reset      every state back to NaN, on `stream`.
 * get_state / set_state   the whole state, float32 [M], to / from the host; both wait for `stream`.
 * set_fence  as rcfm_gate_set_fence: when on, a run waits for the event the previous run of this handle recorded and
 *            records its own.  Off by default, and then no event is touched.
 *
 * rcfm_floor_thresholds.  Stateless: thr[i] = __fmul_rn(floor[cell[i]], gain[i]), i < count; floor [M] float32, cell
 * [count] int32, gain and thr [count] float32, all on the device.  A cell index outside [0, M) gives a NaN threshold --
 * rcfm_squelch and rcfm_gate_run keep such a channel closed -- and nothing is read out of bounds.  RCFM_ERR_ARG before any
 * device call: a NULL pointer, M outside 1 .. 2^30, count < 0, a pointer not aligned for four bytes. */
int rcfm_rank_filter(const void* x, int64_t M, int half, int guard, int q, void* out, void* stream);
int rcfm_floor_create(int64_t M, int half, int guard, int q, float rise, float fall, rcfm_floor_t* out);
int rcfm_floor_run(rcfm_floor_t h, const void* power, float ratio, void* floor, void* over, void* stream);
int rcfm_floor_thresholds(const void* floor, int64_t M, const void* cell, const void* gain, int count, void* thr, void* stream);
int rcfm_floor_reset(rcfm_floor_t h, void* stream);
int rcfm_floor_get_state(rcfm_floor_t h, float* state_host, void* stream);
int rcfm_floor_set_state(rcfm_floor_t h, const float* state_host, void* stream);
int rcfm_floor_set_fence(rcfm_floor_t h, int on);
int rcfm_floor_destroy(rcfm_floor_t h);

/* ---- audio buses: the open channels mixed to a few mono or stereo streams (no reference counterpart) -----------------------
 * Hundreds of channel rows can be recorded, not listened to: a band monitor is heard through a few mixed outputs ("tower +
 * ground + approach on one stream, everything else on a second"), every member at its own gain and spread from left to right
 * so that two talkers who overlap stay separable.  The mixer adds the open rows up on the device; its output is one more
 * [rows][A ch] block with a mask, which rcfm_audio_pack and the drain take as they take the channel rows.
 *
 * Definition.  A mixer has M buses, 1 <= M <= 1024.  Bus m owns routes j = bus_start[m] .. bus_start[m + 1] - 1; a bus may be
 * empty and has at most 65 535 routes; R = bus_start[M] <= 2^20 routes in all.  Route j has a channel index c_j and two
 * float32 gains (gl_j, gr_j), finite.  A channel appears at most once per bus, and in any number of buses.
 * Input: audio [count][A][ch_in] float32, the channels [first, first + count), ch_in 1 or 2; open [count] uint8 as
 * rcfm_squelch / rcfm_gate_run write it, any nonzero byte is open, NULL: every channel is open.
 * Output: out [M][A][ch_out] float32, ch_out 1 or 2; active [M] int32, the number of open routes of each bus; bus_open [M]
 * uint8, 1 where active > 0, else 0.  active and bus_open may be NULL.
 *
 * Terms.  Every product and every sum is one float32 operation, round to nearest, never contracted to an fma: (x) is
 * __fmul_rn, (+) is __fadd_rn.  With x^L, x^R the first and the last leg of the row's sample (the same leg when ch_in = 1):
 *   ch_out = 2:              t^L = gl (x) x^L,  t^R = gr (x) x^R
 *   ch_out = 1, ch_in = 1:   t = gl (x) x
 *   ch_out = 1, ch_in = 2:   t = (gl (x) x^L) (+) (gr (x) x^R)
 *
 * Order.  It depends on the bus's route list alone -- never on the mask, the device, the launch or the alignment.  The
 * routes of a bus are cut by position into segments of 16 consecutive routes (the last may be shorter).  Segment sum:
 * s_k = (..((+0 (+) t_a) (+) t_b)..) over the OPEN routes of segment k in route order.  Output: out = (..((+0 (+) s_0) (+)
 * s_1)..) over all segments in order; a segment with no open route contributes +0.  The rows of a closed route are not read:
 * a NaN in a closed row reaches no output.  A bus with no open route, or with no route at all, gets a row of +0.  The
 * segments are there so that a long route list can be spread over waves; how the work is dealt out is the implementation's
 * choice, the order is not.  No atomics: the output bits are the same from run to run, from stream to stream, and whatever
 * the 4- or 16-byte alignment of audio and out.
 *
 * create    bus_start_host [M + 1], route_channel_host [R], route_gain_host [R][2] (gl, gr); the handle keeps a host copy and
 *           a device copy of the tables, the latter plain device memory that never comes from a bound arena.  It holds no
 *           state across buffers: any number of streams may run it without a fence.  RCFM_ERR_ARG before any device call: a
 *           NULL pointer, M outside 1 .. 1024, ch_out outside {1, 2}, bus_start[0] != 0, a bus_start that decreases, a bus of
 *           more than 65 535 routes, R > 2^20, a negative channel index, a channel twice in one bus, a gain that is not finite.
 * run       One kernel, asynchronous on `stream`, no device allocation, no host synchronisation.  RCFM_ERR_ARG before any
 *           device call: a NULL handle, audio or out, ch_in outside {1, 2}, count < 1, A < 1, audio or out not aligned for a
 *           float (active: for an int32), out overlapping audio.  RCFM_ERR_INDEX when a route's channel lies outside
 *           [first, first + count): the host copy decides, nothing is launched.
 * destroy   NULL is accepted. */
int rcfm_mix_create(int M, const int32_t* bus_start_host, const int32_t* route_channel_host,
                    const float* route_gain_host /* [R][2] */, int ch_out, rcfm_mix_t* out);
int rcfm_mix_run(rcfm_mix_t h, int first, int count, int A, int ch_in, const void* audio, const void* open, void* out,
                 void* active, void* bus_open, void* stream);
int rcfm_mix_destroy(rcfm_mix_t h);

/* ---- bus dynamics: a look-ahead peak limiter and ducking behind the mixer (no reference counterpart) -----------------------
 * The mixer's sum has unit gain: four stations at once leave +-1, and rcfm_audio_pack then clamps, which is hard clipping.
 * This stage knows a peak one block before it arrives and turns the bus down ahead of it, and a side-chain turns one bus
 * down while another one is active ("the tower bus ducks everything else").  It delays every bus by L samples.
 *
 * All arithmetic is float32 and every (+) (-) (x) (/) is one IEEE operation, round to nearest: nothing is contracted to an
 * fma, the division is the correctly rounded one.  Every maximum is "v > p ? v : p" from p = +0, so a NaN never wins;
 * min(a, b) is "b < a ? b : a".
 *
 * A handle has M buses (1 .. 1024) of ch legs (1 or 2); L (8 .. 2048), the block length in samples, which is both the
 * look-ahead and the latency; c, the ceiling, finite and > 0; k in (0, 1], the release coefficient per block; and, optional,
 * per bus m: key[m], -1 or the bus 0 .. M - 1, != m, that ducks bus m; d[m] in (0, 1], the duck depth; thr[m] >= 0, the level
 * of the key bus above which it counts as active; hold[m], 0 .. 2^15, the blocks of hang after the key bus has fallen silent.
 * State per bus: tail [L][ch] float32 (zeros after create and reset), h float32 (1.0), hang int32 (0).
 *
 * run    in [M][A][ch] float32 (the mixer's out), bus_open_in [M] uint8 or NULL (every bus open); writes out [M][A][ch] and
 *        bus_open_out [M] uint8 (may be NULL).  Per bus m:
 *   1. ext[n], n in [-L, A): the tail followed by the row.
 *   2. a[n] = the maximum over the legs of |ext[n]|.
 *   3. B = ceil(A / L) blocks with the edges e_j = min(j L, A).
 *   4. Pk[-1] = the maximum of a over the tail, Pk[j] = the maximum of a over [e_j, e_(j+1)).
 *   5. Knots: h[0] is the state; for b = 1 .. B in order
 *        Q = max(Pk[b-2], Pk[b-1]);  T = Q > c ? c (/) Q : 1;
 *        if key[m] >= 0, with Qk the same maximum over the KEY bus's Pk (its input, never its output: no bus waits for
 *        another bus's result):  Qk > thr[m]: hang = hold[m], ducking is on;  else hang > 0: hang -= 1, ducking is on;
 *        else ducking is off.  While ducking is on, T = min(T, d[m]);
 *        r = h[b-1] (+) ((1 (-) h[b-1]) (x) k);  h[b] = min(T, r).
 *   6. Output: for n in block j, i = n - j L, len = e_(j+1) - e_j:  w = float32(i + 1) (/) float32(len);
 *        g = h[j] (+) ((h[j+1] (-) h[j]) (x) w);  y = ext[n - L][leg] (x) g;  out[n][leg] = y > c ? c : (y < -c ? -c : y).
 *      The clamp is part of the definition: without it the product can exceed c by one ulp.
 *   7. New state: tail = ext[A - L .. A), h = h[B], hang as step 5 left it.
 *   8. bus_open_out[m] = bus_open_in[m] != 0 || Pk[-1] > 0: a bus whose channels have just closed still owes L samples.
 *   9. Every bus runs in every call and its state advances whether or not it is open; an idle bus is a row of +0.
 * Consequences: |out| <= c for every finite input (an infinite or NaN sample comes out as NaN); a row that never exceeds c, with no duck active, comes out as the input delayed by L bit
 * for bit (h = T = r = g = 1 exactly); one call of 2 A equals two calls of A when L divides A; A < L works.
 * Three launches (block peaks, knots -- walked in order, one wave per bus: the recurrence cannot be re-associated -- and apply),
 * asynchronous on `stream`, no atomics, no device allocation, no host synchronisation; the output bits do not depend on the
 * 4- or 16-byte alignment of in and out.
 *
 * create     A_max: the longest row a run may bring (the scratch for Pk and h is sized from it), 1 .. 2^30.  key_host,
 *            depth_host, thr_host, hold_host: [M] each, or key_host NULL: no ducking, and the other three are not read.  A
 *            key chain (a ducks b, b ducks c) is allowed.  RCFM_ERR_ARG before any device call: `out` NULL, M, ch, L, A_max,
 *            ceiling or release_k outside the ranges above (NaN included), a key table without one of the other three, a
 *            key outside -1 .. M - 1 or equal to its own bus, a depth, threshold or hold outside its range.
 * run        RCFM_ERR_ARG before any device call: a NULL handle, in or out, A < 1, A > A_max, in or out not aligned for a
 *            float, out overlapping in.
 * reset      every state back to its value after create, on `stream`.
 * set_fence  as rcfm_gate_set_fence: when on, a run waits for the event the previous run of this handle recorded and
 *            records its own.  Off by default, and then no event is touched.
 * destroy    NULL is accepted.
 * rcfm_tools.h has rcfm_busdyn_state, which copies the state to the host for tests. */
int rcfm_busdyn_create(int M, int ch, int L, int A_max, float ceiling, float release_k, const int32_t* key_host,
                       const float* depth_host, const float* thr_host, const int32_t* hold_host, rcfm_busdyn_t* out);
int rcfm_busdyn_run(rcfm_busdyn_t h, int A, const void* in, const void* bus_open_in, void* out, void* bus_open_out,
                    void* stream);
int rcfm_busdyn_reset(rcfm_busdyn_t h, void* stream);
int rcfm_busdyn_set_fence(rcfm_busdyn_t h, int on);
int rcfm_busdyn_destroy(rcfm_busdyn_t h);

/* ---- noise blanker: impulse noise removed from the wideband buffer, ahead of the FFT (no reference counterpart) -----------
 * A pulse of a few samples (ignition, switching supplies, electric fences) is white across the band: after rcfm_tuner_load it
 * sits in every channel at once and nothing can remove it.  It can be removed where it is still a few samples long, in the
 * time-domain buffer.  A C host calls rcfm_blanker_run before rcfm_tuner_load / rcfm_tuner_load_raw on the same stream; no
 * rcfm_tuner_* entry point knows of it.
 *
 * Input.  n samples of one of four formats: RCFM_IQ_CF32 (complex64) or the three integer formats of rcfm_tuner_load_raw,
 * converted to float32 by the rules given there, which are exact.
 * A handle has
 *   L       the block length, a power of two, 64 <= L <= 2^20;
 *   W       the half-span in blocks, 0 <= W <= 8;
 *   mode    RCFM_BLANK_MEDIAN or RCFM_BLANK_ABSOLUTE, and a double `value`: the threshold ratio (linear, in power) or the
 *           absolute threshold (the power of a sample, full scale 1.0);
 *   H       hold, H >= 0 samples;
 *   ramp[R] float32, supplied by the host, every value in [0, 1], R >= 0;  G = H + R <= 1024.
 * Sample power.  p[i] = fl32(fl32(re re) + fl32(im im)): two products and a sum, each rounded on its own, never an FMA.
 * Block level.  Block b = i >> log2 L, nb = ceil(n / L); the last block may be short.  m[b] is the mean over the block's own
 *   samples of (double)re^2 + (double)im^2, summed in float64 as the pairwise tree over the block's L slots (node j of a
 *   level = node 2 j + node 2 j + 1 of the level below, slots at and beyond n being zero) and divided by the number of
 *   samples: the order is a function of (n, L) alone and there are no floating-point atomics.  A non-finite m[b] counts as +inf.
 * Threshold.  RCFM_BLANK_MEDIAN: r[b] is the lower median of m over blocks max(0, b - W) .. min(nb - 1, b + W), the element
 *   (cnt - 1) / 2 of the ascending sort; t[b] = (float)(value r[b]), one rounding of the float64 product.  A pulse inflates the
 *   mean of its own block many times over, but not the median of nine blocks.  RCFM_BLANK_ABSOLUTE: t[b] = (float)value for
 *   every block; neither the level pass nor the median pass is launched.
 * Hit.  hit[i] = p[i] > t[b(i)]; a NaN on either side gives no hit.
 * Distance.  d[i] = min |i - j| over the hit samples j, infinite where the buffer has none.  Distances do not wrap at the
 *   buffer's ends and nothing is carried from buffer to buffer: the stage has no state, and lanes need no fence.
 * Gain.  g[i] = 0 for d <= H, ramp[d - H - 1] for H < d <= G, 1 beyond G.
 * Output.  g = 1: the sample is copied bit for bit (NaN payloads and -0 survive); with out == in it is not written at all.
 *   g = 0: complex64 stores (+0.0, +0.0), CS16 / CS8 store 0, CU8 stores I = Q = 127 + (i & 1) -- the centre 127.5 is not a
 *   code, and alternating around it leaves no DC step.
 *   otherwise: complex64 stores (fl32(g re), fl32(g im)); CS16 / CS8 store (int)rintf(fl32(g (float)v)) of each integer v;
 *   CU8 stores (int)rintf(fl32(127.5f + fl32(g fl32((float)u - 127.5f)))).
 * Stats.  Optionally a device int64 [2]: the number of hits and the number of samples with g < 1 (integer atomics: counts do
 *   not depend on order).
 * Determinism.  Output and stats are bit-identical from run to run, from stream to stream, in place and out of place, and
 *   wherever the buffers lie within their alignment.
 *
 * create   ramp_host [ramp] (may be NULL when ramp == 0).  The handle owns its scratch -- block sums, thresholds, and the hit
 *          mask of ceil(n_max / 4096) x 128 words -- allocated here, never in run.  RCFM_ERR_ARG before any device call: a NULL
 *          out, n_max outside 1 .. 2^40, a block that is not a power of two or outside 64 .. 2^20, span outside 0 .. 8, an
 *          unknown mode, a value that is not finite or is <= 0, hold < 0, ramp < 0, hold + ramp > 1024, a NULL ramp table
 *          with ramp > 0, a ramp value outside [0, 1] or not finite.
 * run      in -> out, n samples of `format`, asynchronously on `stream`, without a device allocation or a host
 *          synchronisation.  out == in is allowed and is the cheap form (a tile without a hit nearby is not touched); any
 *          other overlap of the two byte ranges is refused.  in and out are aligned for one sample: 8, 4 or 2 bytes; stats
 *          for an int64.  n = 0 is a no-op that zeroes stats.  Runs of ONE handle share its scratch: order them on one
 *          stream at a time (a host with several lanes keeps a handle per lane).
 *          RCFM_ERR_ARG before any device call: a NULL handle or buffer, n < 0 or n > n_max, an unknown format,
 *          misalignment, partial overlap. */
typedef struct rcfm_blanker* rcfm_blanker_t;
enum { RCFM_BLANK_MEDIAN = 0, RCFM_BLANK_ABSOLUTE = 1 };
int rcfm_blanker_create(int64_t n_max, int block, int span, int mode, double value, int hold, const float* ramp_host, int ramp,
                        rcfm_blanker_t* out);
int rcfm_blanker_run(rcfm_blanker_t b, int format, int64_t n, const void* in, void* out, void* stats, void* stream);
int rcfm_blanker_destroy(rcfm_blanker_t b);

/* ---- host ingest (the step before Tuner.load) -------------------------------- */

/* The reference hands its DSP thread a buffer in mapped / shared memory (cusignal.get_shared_mem at
 * radiocore/tools/buffer.py:43 and ringbuffer.py:51; consumer loop examples/multi_fm_server.py:95-98).  Here the
 * host side is page-locked memory and the wideband buffer crosses PCIe once: a feeder owns `depth` device slots of
 * `bytes` each, a copy stream and one event pair per slot, so the copy of buffer i+1 runs under the kernels of
 * buffer i.  device_slots = NULL: the library allocates the slots; otherwise `depth` caller-owned device pointers.
 *   submit(src_host)      queue the H2D copy of the next buffer (page-locked source: rcfm_host_register, or any
 *                         pinned allocation) into the next free slot; RCFM_ERR_STATE when all slots are in flight
 *   acquire(stream, &p)   make `stream` wait for the oldest submitted copy; p = its device slot (pass it to
 *                         rcfm_tuner_load on the same stream)
 *   release(stream)       the work queued on `stream` so far is the last reader of that slot
 *   copied(&count)        how many submitted buffers have LANDED in their slot (host-side query, no wait): source
 *                         buffers [0, count) may be reused or freed by the producer (the RingBuffer's read pointer
 *                         may pass them, ringbuffer.py:129-160)                                              */
int rcfm_host_register(void* host, size_t bytes);
int rcfm_host_unregister(void* host);
int rcfm_feeder_create(size_t bytes, int depth, void* const* device_slots, rcfm_feeder_t* out);
int rcfm_feeder_submit(rcfm_feeder_t f, const void* src_host);
int rcfm_feeder_acquire(rcfm_feeder_t f, void* stream, void** dptr);
int rcfm_feeder_release(rcfm_feeder_t f, void* stream);
int rcfm_feeder_copied(rcfm_feeder_t f, uint64_t* count);
int rcfm_feeder_destroy(rcfm_feeder_t f);

/* ---- host egress (the step after rcfm_audio_pack: the publish loop, examples/multi_fm_server.py:103-106) ------------- */

/* The mirror of the feeder.  A drain owns `depth` slots; a slot is device memory for one rcfm_audio_pack -- packed
 * [max_rows][row_bytes], index [max_rows] int32, n_open -- always plain device memory, never a piece of a bound arena, and
 * a page-locked host mirror of it.  The header (n_open and index, (1 + max_rows) 4 bytes) and the payload travel on two
 * copy streams of the drain, so the compute stream never waits for the host, and per buffer the header plus n_open rows
 * cross PCIe, not max_rows rows.
 *   begin(&packed, &index, &n_open)   device pointers of the next free slot, to pass to rcfm_audio_pack; RCFM_ERR_STATE
 *                                     when all slots are in flight
 *   submit(stream)                    the pack of that slot is queued on `stream`: records an event there, makes the header
 *                                     stream wait for it and queues the header's copy to the host
 *   acquire(&n, &index, &rows)        the oldest submitted slot: waits on the host for its header only, queues the copy of
 *                                     exactly n_open row_bytes payload bytes on the payload stream (nothing when n_open is
 *                                     0) and waits for it; index_host [n_open] and rows_host [n_open][row_bytes] point
 *                                     into the page-locked slot and stay valid until release.  RCFM_ERR_STATE with nothing
 *                                     submitted
 *   release()                         the slot is free again; RCFM_ERR_STATE without an acquired slot
 *   destroy()                         synchronises both copy streams before anything is freed
 * Why two streams: the header copy of buffer i+1 waits for that buffer's kernels; a payload of buffer i queued behind it
 * on the same stream would wait for them too.
 * RCFM_ERR_ARG before any device call: a NULL pointer, row_bytes == 0, max_rows < 1 or > 65535, depth < 1 or > 64. */
typedef struct rcfm_drain_s* rcfm_drain_t;
int rcfm_drain_create(size_t row_bytes, int max_rows, int depth, rcfm_drain_t* out);
int rcfm_drain_begin(rcfm_drain_t d, void** packed_dev, void** index_dev, void** n_open_dev);
int rcfm_drain_submit(rcfm_drain_t d, void* stream);
int rcfm_drain_acquire(rcfm_drain_t d, int* n_open, const int32_t** index_host, const void** rows_host);
int rcfm_drain_release(rcfm_drain_t d);
int rcfm_drain_destroy(rcfm_drain_t d);

/* ---- multi-GPU: the audio gather (the publish step, examples/multi_fm_server.py:103-106) ---------- */

/* One process per GPU; channels shard by contiguous index range (radiocore/tools/sharding.py) and the only
 * collective of the path brings every rank's [C/G][A][ch] float32 block to the publishing rank over xGMI.  RCCL is
 * opened at run time by the first of these calls (a single-GPU process never loads it).
 *   unique_id(id)                 rank 0 creates the 128-byte rendezvous token; the host distributes it to the other
 *                                 ranks by whatever control channel it has (file, socket, MPI, torch.distributed store)
 *   comm_init_rank(G, r, id, &c)  collective: every rank calls it once, with its GPU current (hipSetDevice)
 *   gather_audio(c, root, send, floats, recv, stream)
 *                                 `floats` float32 values from every rank land at recv + rank * floats on `root`
 *                                 (recv may be NULL elsewhere), asynchronously on `stream`: rank blocks are equal,
 *                                 pad the shorter ones when C is not divisible by G (sharding.gather_audio does).  */
#define RCFM_UNIQUE_ID_BYTES 128
int rcfm_comm_unique_id(void* id128_host);
int rcfm_comm_init_rank(int world, int rank, const void* id128_host, rcfm_comm_t* out);
int rcfm_gather_audio(rcfm_comm_t c, int root, const void* send, size_t floats_per_rank, void* recv, void* stream);
/* The rotating FFT owner's hand-over without torch.distributed (Python: radiocore.tools.sharding.SpectrumRing; no
 * reference counterpart -- its one process keeps Tuner._buffer, tuner.py:57,138, to itself).  Rank i mod G runs the
 * wideband FFT of buffer i into a spectrum slot (rcfm_tuner_attach_spectrum + rcfm_tuner_load) and sends every peer the
 * bins that peer's channels read (rcfm_tuner_window: at most two contiguous pieces of the circular spectrum); the peer
 * receives them into the same positions of its own slot and calls rcfm_tuner_adopt.  Point-to-point over xGMI:
 *   group_start / group_end   bracket all sends and receives of one buffer (ncclGroupStart / ncclGroupEnd): they are
 *                             posted together, so no ordering between peers can deadlock
 *   send_bins(c, peer, p, n)  n complex64 bins from device pointer p to rank `peer`, asynchronously on `stream`
 *   recv_bins(c, peer, p, n)  the matching receive.  peer = this rank is allowed inside a group (send + receive to
 *                             itself: a device copy) -- a one-GPU host can run the whole protocol.
 * examples/c_host.c runs it on a one-rank communicator. */
int rcfm_comm_group_start(rcfm_comm_t c);
int rcfm_send_bins(rcfm_comm_t c, int peer, const void* bins, size_t nbins, void* stream);
int rcfm_recv_bins(rcfm_comm_t c, int peer, void* bins, size_t nbins, void* stream);
int rcfm_comm_group_end(rcfm_comm_t c);
int rcfm_comm_destroy(rcfm_comm_t c);

/* ---- primitives (class parity with radiocore/analog) ---------------------- */

/* Limits, checked on the host before anything is launched (RCFM_ERR_ARG beyond them):
 *   C      1 .. 65535 signals per call, for every entry point that takes C (rcfm_resampler_create, rcfm_filtfilt,
 *          rcfm_lfilter_fir, rcfm_agc, rcfm_hilbert, rcfm_discriminator): the signal index is a grid coordinate
 *   ntaps  rcfm_filtfilt 1 .. 2867, rcfm_lfilter_fir 1 .. 5461: the kernels keep the taps and a tile of the signal
 *          in 64 KiB of LDS
 *   count  rcfm_pll_phase: at most 4 294 967 040 samples (one thread each)
 * Arrays are dense: signal c starts at element c * n (c * m for the resampler's output). */

/* Decimate, decimate.py:21-50 = scipy.signal.resample with the fftshifted
 * periodic Hamming window: C signals of n samples -> m samples.
 * is_complex = 0: float32 in/out; 1: complex64 in/out (receive_fm.py:80). */
int rcfm_resampler_create(int C, int n, int m, int is_complex, rcfm_resampler_t* out);
int rcfm_resampler_run(rcfm_resampler_t r, const void* in, void* out, void* stream);
int rcfm_resampler_destroy(rcfm_resampler_t r);

/* Bandpass.run, bandpass.py:59-74 = filtfilt(taps, [1], x), padtype odd:
 * x [C][n] float32 -> y [C][n] float32; taps_host: ntaps float32 (firwin output,
 * designed on the host in both trees, bandpass.py:50-54).  n > 3*ntaps. */
int rcfm_filtfilt(int C, int n, const float* taps_host, int ntaps, const void* x, void* y,
                  void* stream);
/* Deemphasis.run, deemphasis.py:51-66 = lfilter(taps, 1, x, zi=state):
 * x [C][n] -> y [C][n] float32; state [C][ntaps-1] float32 DEVICE, updated in place (one state per signal; may be
 * NULL for ntaps = 1, which has none).  n may be shorter than the state: what is left of it moves up, as in lfilter.
 * NOT in place: x [C][n] and y [C][n] must not overlap; y == x and any partial overlap are refused with RCFM_ERR_ARG
 * (the final state is built from x after y is written, and a tile of y needs the inputs before it). */
int rcfm_lfilter_fir(int C, int n, const float* taps_host, int ntaps, void* state, const void* x,
                     void* y, void* stream);
/* The AGC tail as a primitive (definition: "stateful AGC" above): v [C][n] -> audio [C][n] float32, state [C] float32
 * DEVICE, read and updated in place.  audio == v allowed; any partial overlap is refused. */
int rcfm_agc(int C, int n, int mode, double decay_samples, float level, float floor, void* state, const void* v,
             void* audio, void* stream);
/* PLL.step, pll.py:25-34 = scipy.signal.hilbert: x [C][n] float32 -> z [C][n] complex64. */
int rcfm_hilbert(int C, int n, const void* x, void* z, void* stream);
/* PLL.real / PLL.image, pll.py:36-58: out = Re or Im of z^mult / |z^mult|;
 * z [count] complex64 -> out [count] float32.  Integer mult in [1, 64] is multiplied
 * out like numpy's complex power (and overflows / underflows to NaN like it when |z|^mult leaves float32); any other
 * mult uses the principal branch, cos / sin(mult arg z), whatever |z|.  z = 0 gives NaN, except for mult = 0 (1, 0). */
int rcfm_pll_phase(const void* z, size_t count, double mult, int want_imag, void* out,
                   void* stream);
/* FM discriminator, fm.py:60-65: iq [C][n] complex64 -> d [C][n] float32; d[c][0] = 0 for every signal c (no
 * difference is taken across signals). */
int rcfm_discriminator(int C, int n, const void* iq, void* d, void* stream);

/* ---- FFT engine (the hand-written replacement of cupy.fft / scipy.fft calls) -- */

/* Unnormalised forward (inverse = 0) or conjugate (inverse = 1) transform of `batch`
 * contiguous length-n complex64 signals; in == out allowed.  (scipy.fft.fft / ifft*n) */
int rcfm_fft_c2c(int64_t n, int batch, int inverse, const void* in, void* out, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* RCFM_H */
