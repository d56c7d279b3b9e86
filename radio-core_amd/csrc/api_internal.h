// What the host-side translation units of librcfm.so share (not part of the ABI): the tuner and demodulator handles
// that rcfm_pipeline_run joins, the resampling geometry and plan cache they both hold, the stage profiler every launch
// reports to, and the switches that pick a kernel's tile width or the FFT back end.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "fft_engine.h"
#include "fft_plan.h"
#include "fused_passes.h"
#include "kernels.h"
#include "lds_chain.h"

// A fused_* function in the tile width the launch deserves (csrc/tile_ns.h): 16 lines per tile for batches, 8 for a
// handful of channels.
#define TILE_CALL(narrow_tiles, fn, ...) ((narrow_tiles) ? ::rcfm::narrow::fn(__VA_ARGS__) : ::rcfm::fn(__VA_ARGS__))

namespace rcfm {

constexpr double kPi = 3.14159265358979323846;

// ---- filter and window design (design.hip) ---------------------------------------------------------------------------

// Device tables + scalars of one scipy.signal.resample geometry n -> m.
struct ResampleGeom {
    int64_t n = 0, m = 0;
    int nyq = 0, nneg = 0;
    int nyq_mode = NYQ_NONE;   // complex
    float w_merge = 0.f;       // complex, NYQ_DOWN
    float nyq_factor = 1.f; int nyq_bin = -1;   // real: resample_nyquist (spectrum_rules.h), -1 = no such bin
    float scale = 1.f;         // (m/n) * 1/m for an unnormalised inverse
    DeviceBuffer wpos, wneg;   // complex: float[nyq], float[nneg + 1]
    DeviceBuffer wr;           // real: float[nyq]

    void build(int64_t n_, int64_t m_, double a0, bool complex_input);
};

std::vector<double> firwin_bandpass(int numtaps, double lo, double hi);
std::vector<float> zero_phase_kernel(const float* b, int nb);
void deemphasis_design(int64_t fs, double tau, float* taps51, float* zi50);

// Plans are keyed by batch size: a full chunk and (at most) one remainder.
struct PlanCache {
    std::map<int, std::unique_ptr<FftPlan>> by_batch;
    FftPlan& get(FftKind kind, size_t n, int batch, bool in_place, size_t& work_need) {
        auto it = by_batch.find(batch);
        if (it == by_batch.end())
            it = by_batch.emplace(batch, std::make_unique<FftPlan>(kind, n, (size_t)batch, in_place)).first;
        work_need = std::max(work_need, it->second->work_bytes());
        return *it->second;
    }
};

// ---- per-stage HIP-event timing (profile.hip, rcfm_profile_*) ------------------------------
// bench.py reads these to price the dominant stage against the HBM roofline.
enum Stage : int {
    ST_TUNER_FFT = 0,   // T1  wideband forward FFT
    ST_TUNER_GATHER,    // T2a bin gather + weight
    ST_TUNER_IFFT,      // T2b per-channel inverse FFT
    ST_DISC,            // F1  discriminator (FM/MFM)
    ST_PILOT,           // W1  discriminator + 3-tap + pilot FIR
    ST_FFT_REAL_B,      // r2c of length B (pilot or discriminator)
    ST_HILBERT_MASK,    // W2b
    ST_IFFT_B,          // W2c analytic signal
    ST_STEREO_MIX,      // W3a
    ST_FFT_B,           // W3b packed L/R forward FFT
    ST_AUDIO_SPECTRUM,  // W4a unpack / real spectrum resample
    ST_IFFT_A,          // W4b inverse FFT of length A (c2c packed or c2r)
    ST_DEEMPH,          // W5a FIR51 + partial sums
    ST_DEEMPH_STATE,    // W5b
    ST_DC_CLIP,         // W5c
    ST_LDS_CHAIN,       // T2 + F1 + F2 of narrow FM / MFM channels in one kernel (lds_chain.h)
    ST_ENVELOPE,        // A1  |x| of AM channels (when the tuner did not store it)
    ST_AM_TAIL,         // A2  AM carrier normalisation and clip
    ST_SSB_TAIL,        // S2  SSB RMS normalisation and clip
    ST_LEVELS,          // L1  per-channel signal levels from the loaded spectrum (rcfm_tuner_levels)
    ST_SQUELCH,         // L2  squelch mask and zero fill of closed channels (rcfm_squelch)
    ST_COUNT
};

// One process-wide instance; handles of different threads may time stages concurrently, so every access goes
// through `mu` (uncontended in the single-DSP-thread use the reference has).
struct Profiler {
    std::mutex mu;
    std::atomic<uint64_t> mask{0};
    struct Pair {
        hipEvent_t a, b;
    };
    std::vector<Pair> pending[ST_COUNT];
    std::vector<Pair> pool;
    double total_ms[ST_COUNT] = {};
    int64_t count[ST_COUNT] = {};

    bool on(int st) const { return (mask.load(std::memory_order_relaxed) >> st) & 1u; }
    Pair take() {
        std::lock_guard<std::mutex> lock(mu);
        if (!pool.empty()) {
            Pair p = pool.back();
            pool.pop_back();
            return p;
        }
        Pair p;
        RC_HIP(hipEventCreate(&p.a));
        RC_HIP(hipEventCreate(&p.b));
        return p;
    }
    void push(int st, Pair p) {
        std::lock_guard<std::mutex> lock(mu);
        pending[st].push_back(p);
    }
    void collect() {
        std::lock_guard<std::mutex> lock(mu);
        for (int st = 0; st < ST_COUNT; ++st) {
            for (auto& p : pending[st]) {
                RC_HIP(hipEventSynchronize(p.b));
                float ms = 0.f;
                RC_HIP(hipEventElapsedTime(&ms, p.a, p.b));
                total_ms[st] += ms;
                count[st] += 1;
                pool.push_back(p);
            }
            pending[st].clear();
        }
    }
};

extern Profiler g_prof;

// Brackets one stage (one kernel, or one rocFFT execute) with events on its stream.
struct StageTimer {
    int st;
    hipStream_t s;
    Profiler::Pair p{};
    bool live;
    StageTimer(int stage, hipStream_t stream) : st(stage), s(stream), live(g_prof.on(stage)) {
        if (live) {
            p = g_prof.take();
            RC_HIP(hipEventRecord(p.a, s));
        }
    }
    ~StageTimer() {
        if (live) {
            (void)hipEventRecord(p.b, s);
            g_prof.push(st, p);
        }
    }
};

// ---- which kernels a handle launches --------------------------------------------------------------------------------

// Tile width (RCFM_OPT_NARROW_TILES / RCFM_TUNER_OPT_NARROW_TILES, per handle): 0 = every tile kernel with 16 lines per
// tile, 1 (default) = 8 lines when a launch would leave most CUs without a tile, 2 = always 8.
constexpr int kNarrowDefault = 1;
// RCFM_TUNER_OPT_ALIGNED_PLAN (rcfm_tools.h): 1 = run the aligned order of a wideband plan whose last pass straddles lines.
constexpr int kAlignedPlanDefault = 1;
// One tile per CU and a half-empty chip: that is where a launch lasts one tile's latency and narrower tiles (twice as
// many, half the threads each) shorten it.  From two 16-line tiles per CU on, the wide ones stream better.
inline bool narrow_launch(const FftEngine& e, int signals, int mode) {
    if (mode == 0) return false;
    if (mode >= 2) return true;
    const int64_t tiles = (e.desc().pass[0].n_inner + kFftTileW - 1) / kFftTileW;
    return (int64_t)signals * tiles < 2 * (int64_t)FftEngine::compute_units();
}

// RCFM_FFT=rocfft (environment, read once per process; include/rcfm.h): every transform through rocFFT -- the safety
// net for a host that suspects the engine, and the A/B partner of bench/reference_shapes.py.  The ONLY environment
// variable this library reads.
inline bool use_engine() {
    static const bool v = [] {
        const char* e = std::getenv("RCFM_FFT");
        return !(e && std::string(e) == "rocfft");
    }();
    return v;
}

// Channels [first, first + count) of a handle with n channels.
inline void require_channels(int first, int count, int n) {
    RC_REQUIRE(first >= 0 && count >= 0 && first + count <= n, RCFM_ERR_INDEX, "channel index out of range");
}

}  // namespace rcfm

// ---- the tuner handle (tuner.hip), which rcfm_pipeline_run (demod.hip) reads ----------------------------------------

struct rcfm_tuner_s {
    rcfm::Arena* arena = rcfm::arena_enter_handle();   // rcfm_arena_bind at creation: every workspace of this handle, for its whole life
    ~rcfm_tuner_s() {                                       // (the members drop their pieces after this body)
        if (stage_done) {
            (void)hipEventSynchronize(stage_done);   // a retune's copies may still read the staging memory
            (void)hipEventDestroy(stage_done);
        }
        if (stage) (void)hipHostFree(stage);
        rcfm::arena_leave_handle(arena);
    }
    int opt_narrow = rcfm::kNarrowDefault;  // RCFM_TUNER_OPT_NARROW_TILES (rcfm_pipeline_run passes the demodulator's setting)
    int64_t n = 0;
    int nch = 0;
    std::vector<int64_t> roll;   // normalised to [0, n)
    std::vector<int32_t> bw;
    rcfm::DeviceBuffer roll_dev;
    rcfm::DeviceBuffer base_dev;   // int32 (n - roll) mod n per channel: start of the channel in the haloed spectrum
    // rcfm_tuner_retune: pinned host copy of the new rolls and bases on their way to the device; stage_done is recorded
    // behind the copies, and the next retune waits for it before it overwrites the staging memory
    void* stage = nullptr;
    size_t stage_bytes = 0;
    hipEvent_t stage_done = nullptr;
    rcfm::DeviceBuffer bw_dev;     // int32 bandwidth per channel (rcfm_tuner_levels: a range may mix bandwidths)
    rcfm::DeviceBuffer levels_part;   // rcfm_tuner_levels: float64 [count][segments] sums of channels split over workgroups
    rcfm::DeviceBuffer carriers_part; // rcfm_tuner_carriers: CarrierPart [count][segments] of channels split over workgroups
    rcfm::DeviceBuffer power_part_sum, power_part_max;   // rcfm_tuner_power_spectrum: float64 sums / float32 maxima [cells][segments]
    // rcfm_tuner_set_iq_balance (iq_balance.hip): what every load queues behind its FFT.  The fixed beta and the one the
    // auto mode estimates per buffer live in float32 [2] slots of their own; iq_part: float64 [segments][3] of an estimate
    int iq_mode = RCFM_IQ_BALANCE_OFF;
    int64_t iq_notch = 0;
    rcfm::DeviceBuffer iq_beta_fixed, iq_beta_auto, iq_part;
    rcfm::DeviceBuffer X;          // [halo | n bins | halo]: the halos repeat the far ends, so a channel's bins
    int64_t halo = 0;              //   base + d, |d| <= B/2 + 1, need no wrap-around (fused_passes.h)
    float2* ext = nullptr;         // rcfm_tuner_attach_spectrum: caller-owned storage of the same layout instead of X
    // rcfm_tuner_attach_window: the caller's storage holds [halo | the window's bins | halo] only; `ext` is then the
    // address bin -halo WOULD have (never dereferenced outside the window), and only the window's channels may run
    bool ext_window = false;
    int ext_first = 0, ext_count = 0;
    float2* spectrum() { return (ext ? ext : X.as<float2>()) + halo; }
    rcfm::DeviceBuffer work;
    rcfm::DeviceBuffer forward_work;           // rocFFT fallback of the FORWARD transform: its own workspace -- load() may run on
                                               // another stream than run() (sharding.SpectrumRing), and reserve() may reallocate
    std::unique_ptr<rcfm::FftPlan> forward;    // rocFFT fallback for lengths outside the engine
    std::unique_ptr<rcfm::FftEngine> forward_engine;
    rcfm::DeviceBuffer forward_tmp;            // engine: the last pass cannot run in place
    rcfm::DeviceBuffer raw_c64;                // rcfm_tuner_load_raw without the engine: the converted buffer, [n] complex64,
                                               // reserved by the first such load (a buffer of its own: forward_tmp and the
                                               // rocFFT workspace are busy while the load reads it)
    // rcfm_tuner_load_raw: the conversion rides on the first pass of the wideband FFT (every engine plan has two or more)
    bool raw_fused() const { return forward_engine != nullptr && forward_engine->npass() >= 2; }
    // RCFM_TUNER_OPT_ALIGNED_PLAN: the default plan's pass lengths in the order whose LAST pass stores aligned segments,
    // in the padded-rows layout (fft_engine.h, layout 2) -- N = 2.4e8 = 640 x 625 x 600 with 608-point scratch rows.  Its
    // first intermediate lives in the handle's own spectrum storage (sized for it), so an attached storage runs the
    // default plan.  bin_window() -- the protocol between ranks -- always speaks in rows of the default plan.
    std::unique_ptr<rcfm::FftEngine> forward_aligned;
    int opt_aligned = rcfm::kAlignedPlanDefault;
    rcfm::FftRowWindow window_aligned{0, 0};
    bool windowed_aligned = false;
    size_t own_spectrum_bytes() const {
        int64_t elems = n + 2 * halo;
        if (forward_aligned) elems = std::max<int64_t>(elems, forward_aligned->tmp_stride());
        return sizeof(float2) * (size_t)elems;
    }
    bool use_aligned() const { return forward_aligned && opt_aligned && ext == nullptr && X.bytes() >= own_spectrum_bytes(); }
    rcfm::DeviceBuffer band_tmp;
    bool loaded = false;
    // rcfm_tuner_shard: rows of the spectrum (FftRowWindow) the declared channel range reads
    bool windowed = false;
    rcfm::FftRowWindow window{0, 0};
    int shard_first = 0, shard_count = 0;        // the declared range (valid while windowed)
    // what the spectrum in X was loaded for: a windowed load stores only the rows [loaded_first,
    // loaded_first + loaded_count) reads, so run() refuses channels outside it (the other bins are stale)
    bool loaded_windowed = false;
    int loaded_first = 0, loaded_count = 0;
    void set_loaded(bool now, bool windowed_load, int first, int count) {
        loaded = now;
        loaded_windowed = windowed_load;
        loaded_first = first;
        loaded_count = count;
    }
    // the bins the storage holds since then: [held_first, held_first + held_bins) modulo n (held_bins = n: every bin)
    int64_t held_first = 0, held_bins = 0;
    void set_held(int64_t first_bin, int64_t nbins) {
        held_first = first_bin;
        held_bins = nbins;
    }

    struct Band {
        rcfm::ResampleGeom geom;
        rcfm::PlanCache inverse;
        std::unique_ptr<rcfm::FftEngine> engine;
    };
    std::map<int32_t, std::unique_ptr<Band>> bands;
    Band& band(int32_t b);

    bool row_window(int first, int count, rcfm::FftRowWindow* w, const rcfm::FftEngine* eng = nullptr) const;
    void shard(int first, int count);
    void bin_window(int first, int count, int64_t* first_bin, int64_t* nbins) const;
    void adopt(int first, int count, hipStream_t s);
    void window_storage(int first, int count, int64_t* fb, int64_t* nb) const;
    bool fast_gather_ok(int first);
    bool fast_bins_ok(int32_t B) const;
    bool halo_run_ok(int32_t B) const;
    bool phase_capable(int first);
    int band_row_length(int first);
    bool band_two_pass(int first);
    void require_loaded(int first, int count, const char* caller) const;
    void require_readable(int first, int count, const char* caller, int bw_code, const char* bw_msg) const;
    void levels(int first, int count, float* power, hipStream_t s);
    void carriers(int first, int count, double gate_n2, int32_t* peak_bin, float* peak_power, float* centroid, float* spread,
                  hipStream_t s);
    void retune(int first, int count, const int64_t* roll_host, hipStream_t s);
    void power_spectrum(int64_t s0, int64_t L, int64_t M, float* power, float* peak, hipStream_t s);
    void require_whole(const char* caller) const;
    void iq_estimate(int64_t m_lo, int64_t m_hi, double* sums, float* beta, hipStream_t s);
    void iq_correct(const float* beta, int64_t notch, hipStream_t s);
    void iq_after_load(hipStream_t s);
    void run(int first, int count, float2* out, hipStream_t s, float* theta = nullptr, int theta_pitch = 0,
             int narrow_mode = -1, bool envelope = false);
};
