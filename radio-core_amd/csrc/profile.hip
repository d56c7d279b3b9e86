// Per-stage HIP-event timing (rcfm_profile_*): the Profiler behind every StageTimer (api_internal.h).

#include "api_internal.h"

namespace rcfm {

namespace {
const char* const kStageNames[ST_COUNT] = {
    "tuner_fft_N",   "tuner_gather",  "tuner_ifft_B", "discriminator", "pilot_stage",
    "rfft_B",        "hilbert_mask",  "ifft_B",       "stereo_mix",    "fft_B",
    "audio_spectrum", "ifft_A",       "deemphasis",   "deemph_state",  "dc_clip",
    "lds_chain",     "envelope",      "am_tail",      "ssb_tail",
    "levels",        "squelch"};
}  // namespace

Profiler g_prof;
}  // namespace rcfm

using namespace rcfm;

extern "C" {

int rcfm_profile_stage_count(void) { return ST_COUNT; }

const char* rcfm_profile_stage_name(int stage) {
    return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : "";
}

int rcfm_profile_enable(uint64_t stage_mask) {
    return guarded([&] {
        g_prof.collect();
        g_prof.mask = stage_mask;
    });
}

int rcfm_profile_reset(void) {
    return guarded([&] {
        g_prof.collect();
        std::lock_guard<std::mutex> lock(g_prof.mu);
        for (int i = 0; i < ST_COUNT; ++i) {
            g_prof.total_ms[i] = 0.0;
            g_prof.count[i] = 0;
        }
    });
}

int rcfm_profile_read(int stage, double* total_ms, int64_t* launches) {
    return guarded([&] {
        RC_REQUIRE(stage >= 0 && stage < ST_COUNT && total_ms && launches, RCFM_ERR_ARG, "bad stage");
        g_prof.collect();
        std::lock_guard<std::mutex> lock(g_prof.mu);
        *total_ms = g_prof.total_ms[stage];
        *launches = g_prof.count[stage];
    });
}

}  // extern "C"
