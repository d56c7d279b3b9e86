// The demodulator handle (rcfm_demod_*): the per-chunk kernel chains of FM / MFM / WBFM / AM / USB / LSB.run, one method
// per route a chunk can take, and rcfm_pipeline_run, which joins a tuner to a demodulator.

#include <cmath>
#include <cstring>
#include <optional>

#include "agc.h"
#include "api_internal.h"
#include "pair_scale.h"

using namespace rcfm;

// The per-chunk kernel chains of FM / MFM / WBFM / AM / USB / LSB.run.
struct rcfm_demod_s {
    Arena* arena = arena_enter_handle();   // rcfm_arena_bind at creation
    ~rcfm_demod_s() {
        drop_graphs();
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        arena_leave_handle(arena);
    }
    int kind = 0, C = 0, B = 0, A = 0, ch = 1, chunk = 1;
    double tau = 75e-6;
    float taps_h[51];
    float zi_h[50];
    float pilot_h[41];
    float pilot_g_h[41];   // zero-phase kernel g = b (*) reverse(b), centre first
    DeviceBuffer taps, pilot_g;
    // De-emphasis state, [C][ch][50].  Normally this handle's own buffer; after rcfm_demod_bind_state a
    // one-channel handle's state IS slot `index` of a batched handle's buffer (shared ownership), so the
    // per-channel caller and the batched caller carry ONE state per channel like the reference's
    // Deemphasis._state (deemphasis.py:48-49,64).
    // RCFM_OPT_STATE_FENCE: handles that share one state buffer may run consecutive buffers on DIFFERENT streams (one
    // handle set per stream, radiocore.tools.Lanes).  The fence travels with the buffer (bind_state shares both).
    struct StateBuf : DeviceBuffer {
        StreamFence fence;
    };
    std::shared_ptr<StateBuf> state_buf = std::make_shared<StateBuf>();
    size_t state_off = 0;   // floats into state_buf
    float* state_ptr() const { return state_buf->as<float>() + state_off; }
    float* state_at(int first) const { return state_ptr() + (size_t)first * state_stride(); }   // channel `first`'s slot
    float side_tap = 0.23f;
    ResampleGeom geom;   // B -> A, real, Hamming
    PlanCache r2c_B, c2c_inv_B, c2c_fwd_B, c2c_inv_A, c2r_A;
    std::unique_ptr<FftEngine> eng_B, eng_A;   // both set: the engine path with fused passes
    std::unique_ptr<FftEngine> eng_Ad;         // length A as (A / n_1, n_1): its first pass tiles like eng_B's last
    std::unique_ptr<FftEngine> eng_Bi;         // eng_B's two pass lengths swapped (k_fft_tile2 pairing)
    DeviceBuffer buf_Ti;
    // rcfm_demod_set_option: which forms of the chain rcfm_pipeline_run / run_chunk may use (all on by default).  Parity
    // tests flip them per handle to get a second evaluation that shares no kernel schedule with the default one; the
    // A/B tools isolate one fusion at a time (RCFM_OPT_PILOT_CHAIN / RCFM_OPT_DECIM_TILE; RCFM_OPT_FUSED_TILES sets both).
    bool opt_lds_chain = true;
    bool opt_pilot_chain = true;     // pilot chain, Hilbert pair / packed tiles (two transforms per tile around the mask)
    bool opt_decim_tile = true;      // spectral decimation between FFT_B's last pass and IFFT_A's first
    bool opt_pilot_blocked = true;   // m, p between the pilot stage and the pilot chain in the tile-blocked layout
    bool opt_phase_link = true;
    bool opt_lds_deemph = true;      // MFM's de-emphasis inside the LDS chain
    bool opt_ssb_direct = true;      // USB / LSB in rcfm_pipeline_run: audio straight from the tuner's spectrum
    int opt_narrow = kNarrowDefault;   // RCFM_OPT_NARROW_TILES
    // RCFM_OPT_GRAPH: one channel per call (the reference's per-channel demodulator.run, tests/benchmark.py:29-31) is ten
    // launches of a few microseconds each: launch-bound.  The second call with the same pointers captures the chain
    // into a hipGraph (the first one has warmed up every lazily built table and workspace, so the capture allocates
    // nothing); later calls replay it with ONE graph launch on the caller's stream.  Same kernels, same arguments:
    // bit-identical.  Not used while a stage timer or the state fence (events on the stream) is on.
    // OFF by default: measured on MI355X / ROCm 7 (profiles/r06_a_single_call.txt) a graph launch of the ten-kernel WBFM
    // chain costs what the ten stream launches cost (73.4 vs 74.8 us synchronous, 61.0 vs 57.8 us queued), and the
    // shorter MFM / FM chains lose 4 - 6 us per call: this runtime's graph launch is no cheaper than its kernel launches.
    bool opt_graph = false;
    struct GraphSlot {
        const void* iq;
        void* audio;
        const float* state;
        int first;
        hipGraphExec_t exec;
        uint64_t used;
    };
    std::vector<GraphSlot> graphs;
    GraphSlot last_call{nullptr, nullptr, nullptr, -1, nullptr, 0};
    hipStream_t cap_stream = nullptr;
    uint64_t graph_tick = 0;
    void drop_graphs() {   // whatever the captured chains depended on has changed (option, state binding)
        for (auto& g : graphs) (void)hipGraphExecDestroy(g.exec);
        graphs.clear();
        last_call = GraphSlot{nullptr, nullptr, nullptr, -1, nullptr, 0};
    }
    bool narrow(int cnt) const { return eng_B && narrow_launch(*eng_B, cnt, opt_narrow); }
    DeviceBuffer work, buf_iq, buf_m, buf_p, buf_P, buf_Z, buf_V, buf_v, partial, buf_T, buf_TA, buf_U2, buf_dc;
    DeviceBuffer buf_scale;   // AM / USB / LSB on the engine: [2][chunk] per-row powers of two and their inverses (pair_scale.h)
    int tiles = 0;

    // Length A as (A / n_1, n_1), n_1 = eb's first pass length, so that its first pass tiles like eb's last and the
    // decimation B -> A rides between the two (fused_passes.h): A = n_1 L2 with L2 even and >= 16, and a plan for it.
    bool decim_plan(const FftEngine& eb, int64_t fa[2]) const {
        const int64_t n1 = eb.desc().pass[0].L;
        fa[0] = A / n1;
        fa[1] = n1;
        FftPlanDesc pa;
        return A % (2 * n1) == 0 && A / n1 >= 16 && fft_plan_describe(A, &pa, 0, fa, 2);
    }

    // MFM and WBFM carry de-emphasis state from buffer to buffer; FM, AM, USB and LSB carry none.
    bool stateful() const { return kind == RCFM_MFM || kind == RCFM_WBFM; }
    bool ssb() const { return kind == RCFM_USB || kind == RCFM_LSB; }

    // rcfm_demod_set_agc (AM, USB, LSB): the AGC tail instead of the per-buffer normalisation.  Its state -- one float
    // per channel, -1 = no history -- lives in state_buf like the de-emphasis state of MFM / WBFM, so binding and the
    // fence treat both alike; a handle's kind decides the stride of a channel's slot.
    bool agc_on = false;
    double agc_decay = 0.0;
    float agc_level = 0.f, agc_floor = 0.f;
    bool carries_state() const { return stateful() || agc_on; }
    size_t state_stride() const { return stateful() ? (size_t)ch * 50 : 1; }   // floats per channel
    // scale_chunk: the rows of `audio` still carry the pair scaling of a chunk of that many channels (0: none); it comes
    // out first, exactly, so that the follower and the state it carries stay in the signal's own units.
    void agc_tail(int first, int cnt, float* audio, hipStream_t s, int scale_chunk) {
        StreamFence::Scope fenced(state_buf->fence, s);
        StageTimer tm(kind == RCFM_AM ? ST_AM_TAIL : ST_SSB_TAIL, s);
        if (scale_chunk) launch_rows_rescale(audio, A, cnt, buf_scale.as<float>() + scale_chunk, s);
        launch_agc_tail(kind == RCFM_AM ? RCFM_AGC_CARRIER : RCFM_AGC_PEAK, audio, audio, A, cnt,
                        agc_params(agc_decay, agc_level, agc_floor), state_at(first), s);
    }

    void alloc() {
        const size_t c = (size_t)chunk;
        tiles = fir_tiles(A);

        if (ssb()) {
            // linear from spectrum to audio: no real-signal buffers.  The engine serves each length it has a plan for
            // (the spectrum-direct route needs A only); route 2 takes rocFFT for both transforms unless both are there.
            FftPlanDesc probe;
            if (use_engine() && fft_plan_describe(A, &probe)) {
                eng_A = std::make_unique<FftEngine>(A);
                buf_TA.reset(((c + 1) / 2) * eng_A->tmp_stride() * sizeof(float2));
            }
            if (eng_A && fft_plan_describe(B, &probe)) eng_B = std::make_unique<FftEngine>(B);
            if (eng_A) buf_scale.reset(2 * c * sizeof(float));
            return;
        }
        if (kind == RCFM_WBFM) {
            buf_P.reset(c * (B / 2 + 1) * sizeof(float2));
            buf_Z.reset(c * B * sizeof(float2));      // analytic pilot, then the packed L/R signal
            buf_V.reset(c * A * sizeof(float2));      // packed audio spectrum -> l + j r
        } else {
            buf_m.reset(c * B * sizeof(float));                    // discriminator output (AM: the envelope)
            buf_P.reset(c * (B / 2 + 1) * sizeof(float2));          // its half spectrum
            buf_V.reset(c * (A / 2 + 1) * sizeof(float2));          // resampled half spectrum
            if (kind == RCFM_MFM) buf_v.reset(c * A * sizeof(float));
        }
        if (stateful()) partial.reset((size_t)chunk * ch * tiles * sizeof(float));
        buf_dc.reset((size_t)chunk * sizeof(float2));
        FftPlanDesc probe;
        if (use_engine() && fft_plan_describe(B, &probe) && fft_plan_describe(A, &probe)) {
            eng_B = std::make_unique<FftEngine>(B);
            eng_A = std::make_unique<FftEngine>(A);
            // Two-pass plans (n_1, L): the decimation B -> A rides between FFT_B's last pass and IFFT_A's first when
            // A = n_1 L2 with L2 even (k_fft_tile2_decim); if the planner's order of the two factors does not allow that
            // and the other order does (256 000 -> 32 000: 512 x 500 gives L2 = 62.5, 500 x 512 gives 64), take the other
            // one -- the fused chain uses both orders of the plan anyway (eng_Bi below).
            if (eng_B->npass() == 2 && A < B) {
                const FftPlanDesc& pd = eng_B->desc();
                auto decim_ok = [&](const FftEngine& eb) {
                    int64_t fa[2];
                    if (!decim_plan(eb, fa)) return false;
                    FftEngine ea(A, fa, 2);
                    return fused_fft_decim_ifft_applies(eb, ea, 1);
                };
                if (!decim_ok(*eng_B)) {
                    const int64_t swapped[2] = {pd.pass[1].L, pd.pass[0].L};
                    FftPlanDesc ps;
                    if (fft_plan_describe(B, &ps, 0, swapped, 2)) {
                        auto alt = std::make_unique<FftEngine>(B, swapped, 2);
                        if (decim_ok(*alt)) eng_B = std::move(alt);
                    }
                }
            }
            buf_T.reset(c * eng_B->tmp_stride() * sizeof(float2));
            buf_TA.reset(c * eng_A->tmp_stride() * sizeof(float2));
            if (kind == RCFM_AM) buf_scale.reset(2 * c * sizeof(float));
            if (kind == RCFM_WBFM) {
                buf_U2.reset(((c + 1) / 2) * B * sizeof(float2));
                const FftPlanDesc& pd = eng_B->desc();
                if (pd.npass == 2) {
                    const int64_t swapped[2] = {pd.pass[1].L, pd.pass[0].L};
                    eng_Bi = std::make_unique<FftEngine>(B, swapped, 2);
                    buf_Ti.reset(c * eng_Bi->tmp_stride() * sizeof(float2));
                }
            }
            int64_t fa[2];   // decimation between FFT_B's last pass and IFFT_A's first (fused_passes.h)
            if (eng_B->desc().npass == 2 && A < B && decim_plan(*eng_B, fa)) {
                eng_Ad = std::make_unique<FftEngine>(A, fa, 2);
                buf_TA.reserve(c * eng_Ad->tmp_stride() * sizeof(float2));
                if (const int pitch = audio_pitch())   // padded rows of the packed audio
                    buf_V.reserve(c * (size_t)(A / eng_Ad->row_length()) * pitch * sizeof(float2));
            }
            if (kind != RCFM_WBFM) {
                buf_Z.reset(c * B * sizeof(float2));   // full spectrum of the discriminator output
                buf_V.reset(c * A * sizeof(float2));   // Hermitian audio spectrum
            }
        }
        if (kind == RCFM_WBFM) {
            // mono signal and pilot band (after the engines: the tile-blocked layout of the pilot chain pads the last
            // 16-column block of every row, PilotBlocked::stride >= B)
            const size_t per_channel = std::max<size_t>((size_t)B, (size_t)pilot_blocked().stride);
            buf_m.reset(c * per_channel * sizeof(float));
            buf_p.reset(c * per_channel * sizeof(float));
        }
    }

    void reset_state(hipStream_t s) {
        if (agc_on) {
            const std::vector<float> all((size_t)C, -1.f);
            RC_HIP(hipMemcpyAsync(state_ptr(), all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice, s));
            RC_HIP(hipStreamSynchronize(s));
        }
        if (!stateful()) return;
        std::vector<float> all((size_t)C * ch * 50);
        for (size_t i = 0; i < all.size(); ++i) all[i] = zi_h[i % 50];
        RC_HIP(hipMemcpyAsync(state_ptr(), all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice, s));
        RC_HIP(hipStreamSynchronize(s));
    }

    // Can run_deemph take its input in padded rows (fused_fft_decim_ifft's out_pitch)?  Only the fused kernel does.
    bool deemph_fused() const { return ((int64_t)A * ch) % 4 == 0 && A >= 50; }
    // Row pitch (samples) of the packed audio between IFFT_A's last pass and the de-emphasis kernel: rows of n_1
    // samples padded to whole 128-byte lines; 0 = contiguous.
    int audio_pitch() const {
        if (!eng_Ad || kind != RCFM_WBFM || !deemph_fused()) return 0;
        const int64_t n1 = eng_Ad->row_length();
        return (n1 % 16 == 0 || (n1 * 2) % 4 != 0) ? 0 : (int)((n1 + 15) / 16 * 16);
    }

    // Are the 51 taps the first samples of a one-pole impulse response (b[0] = 0, geometric tail)?  The same test
    // launch_fir51 applies (kernels.hip): the recursive forms of the FIR rely on it.
    bool deemph_geometric() const {
        if (!(taps_h[0] == 0.f && taps_h[1] > 0.f)) return false;
        for (int i = 1; i < 50; ++i)
            if (std::fabs((double)taps_h[i + 1] * taps_h[1] - (double)taps_h[i] * taps_h[2]) >
                4e-7 * (double)taps_h[i] * taps_h[1] + 1e-36)
                return false;
        return true;
    }

    DeviceBuffer taps_sfx;
    // The taps followed by their suffix sums sfx[i] = sum_{j > i} b[j] (what the on-chip de-emphasis of lds_chain.hip reads).
    const float* taps_sfx_dev() {
        if (taps_sfx.bytes() == 0) {
            float h[102];
            for (int i = 0; i < 51; ++i) h[i] = taps_h[i];
            double acc = 0.0;
            for (int i = 50; i >= 0; --i) {
                h[51 + i] = (float)acc;          // sum of b[j], j > i
                acc += (double)taps_h[i];
            }
            taps_sfx.upload(h, sizeof(h));
        }
        return taps_sfx.as<float>();
    }

    // mfm.py:63-65 / wbfm.py:90-100: de-emphasis of channels [first, first + cnt) (per-leg state), joint DC removal, clip.
    // The mean comes from the DC bin the previous stage left in buf_dc.  generic_fir: that stage left none (the rocFFT
    // routes), so the generic FIR and its partial sums run whatever A is.
    void run_deemph(const float* v, float* audio, int first, int cnt, hipStream_t s, bool generic_fir = false,
                        int row = 0, int pitch = 0) {
        float* st = state_at(first);
        const bool fast = !generic_fir && ((int64_t)A * ch) % 4 == 0;
        StreamFence::Scope fenced(state_buf->fence, s);
        if (fast && A >= 50) {
            // de-emphasis, DC removal and clip in one kernel: the mean comes from the DC bin (buf_dc)
            {
                StageTimer tm(ST_DEEMPH, s);
                launch_fir51(v, audio, A, ch, cnt, taps_h, st, nullptr, buf_dc.as<float2>(), s, row, pitch);
            }
            StageTimer tm(ST_DEEMPH_STATE, s);
            launch_fir_state(v, A, ch, cnt, taps.as<float>(), 51, st, s, row, pitch);
            return;
        }
        RC_REQUIRE(pitch == 0, RCFM_ERR_RUNTIME, "padded audio rows need the fused de-emphasis kernel");
        {
            StageTimer tm(ST_DEEMPH, s);
            if (fast)
                launch_fir51(v, audio, A, ch, cnt, taps_h, st, partial.as<float>(), nullptr, s);
            else
                launch_fir(v, audio, A, ch, cnt, taps.as<float>(), 51, st, partial.as<float>(), s);
        }
        {
            StageTimer tm(ST_DEEMPH_STATE, s);
            launch_fir_state(v, A, ch, cnt, taps.as<float>(), 51, st, s);
        }
        {
            StageTimer tm(ST_DC_CLIP, s);
            launch_dc_clip(audio, A, ch, cnt, partial.as<float>(), fast ? fir51_tiles(A, ch) : tiles * ch, s);
        }
    }

    // The tile-blocked layout of m and p (kernels.h) when the pilot chain's geometry allows it, else an invalid one.
    PilotBlocked pilot_blocked() const {
        int64_t rows = 0, row_length = 0;
        if (kind != RCFM_WBFM || !eng_B || !eng_Bi || B % 4 != 0 || !fused_pilot_chain_geometry(*eng_B, &rows, &row_length))
            return PilotBlocked{};
        return PilotBlocked::plan(rows, row_length);
    }

    // Does run_chunk take the samples' phases (theta = angle(x) / pi, float32 [cnt][B]) instead of iq?
    // AM never: its chain starts from |x|, which the phases do not hold (the tuner stores the envelope for it instead).
    // USB / LSB never either: they need the samples' amplitudes as much as their phases.
    bool phase_capable() const {
        return eng_B != nullptr && kind != RCFM_AM && !ssb() && (kind != RCFM_WBFM || B % 4 == 0);
    }

    // One chunk of channels [first, first + cnt) from iq (or the tuner's phases) to audio, by one of the routes below.
    void run_chunk(int first, int cnt, const float2* iq, float* audio, hipStream_t s, const float* theta = nullptr,
                   PhaseRows rows = PhaseRows{}) {
        if (kind == RCFM_WBFM) {
            if (eng_B)
                run_wbfm_engine(first, cnt, iq, audio, s, theta);
            else
                run_wbfm_rocfft(first, cnt, iq, audio, s, theta);
            return;
        }
        if (kind == RCFM_AM) {
            run_am(first, cnt, iq, audio, s, false);
            return;
        }
        if (ssb()) {
            run_ssb(first, cnt, iq, audio, s);
            return;
        }
        // fm.py:60-66  discriminator, then Decimate(B -> A) into the audio (FM) or into v, which mfm.py:63-65 de-emphasises
        if (theta == nullptr) {
            StageTimer tm(ST_DISC, s);
            launch_discriminator(iq, buf_m.as<float>(), B, cnt, s);
        }
        float* dst = (kind == RCFM_FM) ? audio : buf_v.as<float>();
        run_real(cnt, dst, s, theta, rows);
        if (kind == RCFM_MFM) run_deemph(dst, audio, first, cnt, s, /*generic_fir=*/!eng_B);   // rocFFT left no DC bin
    }

    // Decimate(B -> A) of the real signals in buf_m (or of the phase steps of theta) into dst, by the first route that
    // applies: the decimating tile, the engine with a separate resample, rocFFT.  The engine routes leave the DC bin of
    // every channel's resampled spectrum in buf_dc; rocFFT leaves none (returns false).
    bool run_real(int cnt, float* dst, hipStream_t s, const float* theta, PhaseRows rows) {
        if (eng_B && eng_Ad && opt_decim_tile && ((int64_t)A % 4 == 0 || kind != RCFM_MFM) &&
            TILE_CALL(narrow(cnt), fused_fft_decim_ifft_applies, *eng_B, *eng_Ad, (cnt + 1) / 2))
            run_pair_decim(cnt, dst, s, theta, rows);
        else if (eng_B)
            run_fm_engine(cnt, dst, s, theta, rows);
        else {
            run_fm_rocfft(cnt, dst, s);
            return false;
        }
        return true;
    }

    // AM (include/rcfm.h, RCFM_AM): envelope |x| into buf_m -- unless the tuner's last pass already stored it there
    // (envelope_ready, rcfm_pipeline_run) --, FM's real-signal routes straight into the audio, then the carrier
    // normalisation in place.  Its mean comes from the DC bin when the route left one.
    // The engine routes transform the envelopes two by two, and envelopes stand at their stations' RF levels: each row
    // is brought to [1, 2) by a power of two first (pair_scale.h), which the division by the row's mean cancels.  A
    // chunk of one channel has no partner, and rocFFT transforms row by row.
    void run_am(int first, int cnt, const float2* iq, float* audio, hipStream_t s, bool envelope_ready) {
        const bool scaled = pair_scaled(cnt);
        {
            std::optional<StageTimer> tm;   // the scaling is timed with the envelope kernel it follows
            if (!envelope_ready) {
                tm.emplace(ST_ENVELOPE, s);
                launch_envelope(iq, buf_m.as<float>(), (int64_t)cnt * B, s);
            }
            if (scaled) launch_am_pair_scale(buf_m.as<float>(), B, cnt, buf_scale.as<float>(), s);
        }
        const bool dc = run_real(cnt, audio, s, nullptr, PhaseRows{});
        if (agc_on) {
            agc_tail(first, cnt, audio, s, scaled ? cnt : 0);
            return;
        }
        StageTimer tm(ST_AM_TAIL, s);
        launch_am_tail(audio, A, cnt, dc ? buf_dc.as<float2>() : nullptr, s);
    }

    // AM / USB / LSB: does a chunk of cnt channels go through transforms that two channels share?
    bool pair_scaled(int cnt) const { return cnt > 1 && buf_scale.bytes() != 0; }

    // USB / LSB (include/rcfm.h): where the sideband's spectrum comes from, for fused_ssb_ifft.  The inverse transform
    // carries Y0 + j Y1 of two channels at their stations' levels: with more than one channel in the chunk the load
    // multiplies each by its own power of two (pair_scale.h), found here from the bins it will read; the division by
    // the row's RMS cancels it.
    SsbSource ssb_source(const float2* X, const int32_t* base32, int64_t N, int cnt, hipStream_t s) const {
        SsbSource src{X, base32, N, B, kind == RCFM_LSB, geom.wr.as<float>(), geom.nyq_bin, geom.nyq_factor};
        if (pair_scaled(cnt)) {
            launch_ssb_pair_scale(X, base32, B, (int)std::min<int64_t>(A / 2, (B - 1) / 2), src.lower, cnt,
                                  buf_scale.as<float>(), s);
            src.row_scale = buf_scale.as<float>();
        }
        return src;
    }

    void ssb_tail(int first, int cnt, float* audio, hipStream_t s, bool scaled) {
        if (agc_on) {
            agc_tail(first, cnt, audio, s, scaled ? cnt : 0);
            return;
        }
        StageTimer tm(ST_SSB_TAIL, s);
        launch_ssb_tail(audio, A, cnt, RCFM_SSB_LEVEL, s);
    }

    // USB / LSB, route 1 (rcfm_pipeline_run only): the audio of channels [first, first + cnt) straight from the tuner's
    // loaded spectrum -- IFFT_A of bins picked and weighted on the load, two channels per transform, then the tail.
    // Neither the tuner's IFFT_B nor any B-point transform or resample of this handle runs.
    bool ssb_direct_ok(rcfm_tuner_s& t, int first) const {
        return ssb() && opt_ssb_direct && eng_A && A <= B && t.fast_gather_ok(first);
    }
    void run_ssb_direct(rcfm_tuner_s& t, int first, int cnt, float* audio, hipStream_t s) {
        t.require_readable(first, cnt, "rcfm_pipeline_run", RCFM_ERR_SIZE, "input_sig size and input_size mismatch");
        {
            StageTimer tm(ST_IFFT_A, s);
            TILE_CALL(narrow_launch(*eng_A, (cnt + 1) / 2, opt_narrow), fused_ssb_ifft, *eng_A,
                      ssb_source(t.spectrum(), t.base_dev.as<int32_t>() + first, t.n, cnt, s), audio, buf_TA.as<float2>(), cnt, s);
        }
        ssb_tail(first, cnt, audio, s, pair_scaled(cnt));
    }

    // USB / LSB, route 2, from channel samples: FFT_B keeping |k| <= min(A, B) / 2, then the same inverse transform
    // reading those spectra; lengths outside the engine take rocFFT around a select-and-weight kernel.
    void run_ssb(int first, int cnt, const float2* iq, float* audio, hipStream_t s) {
        if (eng_B && eng_A) {
            buf_Z.reserve((size_t)chunk * B * sizeof(float2));
            buf_T.reserve((size_t)chunk * eng_B->tmp_stride() * sizeof(float2));
            {
                StageTimer tm(ST_FFT_B, s);
                TILE_CALL(narrow(cnt), fused_fft_pruned, *eng_B, iq, buf_Z.as<float2>(), buf_T.as<float2>(), cnt,
                          std::min(A, B) / 2, s);
            }
            StageTimer tm(ST_IFFT_A, s);
            TILE_CALL(narrow_launch(*eng_A, (cnt + 1) / 2, opt_narrow), fused_ssb_ifft, *eng_A,
                      ssb_source(buf_Z.as<float2>(), nullptr, B, cnt, s), audio, buf_TA.as<float2>(), cnt, s);
        } else {
            size_t need = 0;
            FftPlan& f1 = c2c_fwd_B.get(FftKind::C2C_FORWARD, B, cnt, false, need);
            FftPlan& f2 = c2r_A.get(FftKind::C2R, A, cnt, false, need);
            work.reserve(need);
            buf_Z.reserve((size_t)chunk * B * sizeof(float2));
            buf_V.reserve((size_t)chunk * (A / 2 + 1) * sizeof(float2));
            {
                StageTimer tm(ST_FFT_B, s);
                f1.exec(const_cast<float2*>(iq), buf_Z.get(), work.get(), s);   // out of place: iq is only read
            }
            {
                StageTimer tm(ST_AUDIO_SPECTRUM, s);
                launch_ssb_select(buf_Z.as<float2>(), B, buf_V.as<float2>(), A, cnt, geom.wr.as<float>(),
                                  (int)std::min<int64_t>(A / 2, (B - 1) / 2), geom.nyq_bin, geom.nyq_factor, geom.scale, kind == RCFM_LSB, s);
            }
            StageTimer tm(ST_IFFT_A, s);
            f2.exec(buf_V.get(), audio, work.get(), s);
        }
        ssb_tail(first, cnt, audio, s, eng_B && eng_A && pair_scaled(cnt));
    }

    // wbfm.py:77-80  FM(B->B) and the pilot band-pass
    void pilot_stage(const float2* iq, const float* theta, int cnt, const PilotBlocked& blk, hipStream_t s) {
        float* m = buf_m.as<float>();
        float* p = buf_p.as<float>();
        StageTimer tm(ST_PILOT, s);
        if (theta != nullptr)
            launch_pilot_stage_h40_phase(theta, m, p, B, cnt, pilot_g_h, side_tap, s, &blk);
        else if (B % 4 == 0)
            launch_pilot_stage_h40(iq, m, p, B, cnt, pilot_g_h, side_tap, s, &blk);
        else
            launch_pilot_stage(iq, nullptr, m, p, B, cnt, pilot_g.as<float>(), 40, side_tap, s);
    }

    // WBFM on the FFT engine: pilot chain, packed or pair Hilbert tiles, or the separate transforms around the mask; then
    // the decimating tile or a separate IFFT_A.
    void run_wbfm_engine(int first, int cnt, const float2* iq, float* audio, hipStream_t s, const float* theta) {
        const bool nw = narrow(cnt);   // 8-line tiles for a handful of channels (tile_ns.h)
        float* m = buf_m.as<float>();
        float* p = buf_p.as<float>();
        float2* Z = buf_Z.as<float2>();
        float2* V = buf_V.as<float2>();
        float2* T = buf_T.as<float2>();
        float2* TA = buf_TA.as<float2>();
        float2* U2 = buf_U2.as<float2>();
        // the three-launch pilot chain reads m and p as 16-line tiles: they leave the pilot stage tile-blocked then
        const bool chain = eng_Bi && opt_pilot_chain && TILE_CALL(nw, fused_pilot_chain_applies, *eng_B, *eng_Bi, cnt);
        const PilotBlocked blk = (chain && opt_pilot_blocked) ? pilot_blocked() : PilotBlocked{};
        pilot_stage(iq, theta, cnt, blk, s);
        // RCFM_OPT_PILOT_CHAIN = 0: pair FFT -> U2 -> masked IFFT as separate transforms
        const bool packed = eng_Bi && opt_pilot_chain && TILE_CALL(nw, fused_hilbert_packed_applies, *eng_Bi, *eng_B, cnt);
        bool paired = false;
        if (chain) {
            {   // wbfm.py:80 / pll.py:34: spectra of the pilot bands, two channels per complex FFT
                StageTimer tm(ST_FFT_REAL_B, s);
                TILE_CALL(nw, fused_pilot_chain_fft_first, *eng_B, p, T, cnt, s, blk.stride, blk.blk16());
            }
            {   // ... last pass, one-sided mask, inverse FFT, stereo matrix, first pass of the packed L/R FFT
                StageTimer tm(ST_IFFT_B, s);
                TILE_CALL(nw, fused_pilot_chain_mask_mix, *eng_B, *eng_Bi, p, m, T, buf_Ti.as<float2>(), cnt, s, blk.stride,
                          blk.blk16());
            }
            paired = true;
        } else {
            {   // wbfm.py:80 / pll.py:34: spectra of the pilot bands, two channels per complex FFT
                StageTimer tm(ST_FFT_REAL_B, s);
                TILE_CALL(nw, fused_real_pair_fft, *eng_B, p, U2, T, cnt, packed ? kKeepLowerHalf : -1, s);
            }
            if (eng_Bi && opt_pilot_chain) {
                // one-sided mask -> inverse FFT -> stereo matrix -> first pass of the packed L/R FFT:
                // the last IFFT pass and the first FFT pass share their tiles (fused_passes.h)
                StageTimer tm(ST_IFFT_B, s);
                paired = !packed ? TILE_CALL(nw, fused_hilbert_pair_ifft_mix_fft, *eng_Bi, *eng_B, U2, m, buf_Ti.as<float2>(), T, cnt, s)
                                 : TILE_CALL(nw, fused_hilbert_packed_ifft_mix_fft, *eng_Bi, *eng_B, U2, p, m,
                                             buf_Ti.as<float2>(), T, cnt, s);
            }
        }
        if (paired && eng_Ad && opt_decim_tile && TILE_CALL(nw, fused_fft_decim_ifft_applies, *eng_B, *eng_Ad, cnt)) {
            const int pitch = audio_pitch();
            {   // packed L/R FFT last pass -> decimation -> IFFT_A: the B-point spectrum stays on chip
                StageTimer tm(ST_FFT_B, s);
                TILE_CALL(nw, fused_fft_decim_ifft, *eng_B, *eng_Ad, T, V, TA, cnt, geom.wr.as<float>(), geom.scale,
                          buf_dc.as<float2>(), s, pitch);
            }
            run_deemph(reinterpret_cast<float*>(V), audio, first, cnt, s, false, pitch ? (int)eng_Ad->row_length() : 0, pitch);
            return;
        }
        if (paired) {
            StageTimer tm(ST_FFT_B, s);
            TILE_CALL(nw, fused_fft_last_pruned, *eng_B, T, Z, cnt, std::min(A, B) / 2, s);
        } else {
            {   // one-sided mask -> inverse FFT -> 38 kHz carrier, L-R, stereo matrix (wbfm.py:83,86-87)
                StageTimer tm(ST_IFFT_B, s);
                TILE_CALL(nw, fused_hilbert_pair_ifft_mix, *eng_B, U2, m, Z, T, cnt, s);
            }
            {   // both stereo legs in one complex FFT; only |k| <= A/2 survives the decimation
                StageTimer tm(ST_FFT_B, s);
                TILE_CALL(nw, fused_fft_pruned, *eng_B, Z, Z, T, cnt, std::min(A, B) / 2, s);
            }
        }
        {   // unpack + window + Nyquist rule ride on the first pass of IFFT_A
            StageTimer tm(ST_IFFT_A, s);
            TILE_CALL(nw, fused_stereo_unpack_ifft, *eng_A, Z, B, V, TA, cnt, geom.wr.as<float>(), geom.nyq, geom.nyq_bin,
                      geom.nyq_factor, geom.scale, buf_dc.as<float2>(), s);
            // -> [cnt][A][2] float32, L/R interleaved
        }
        run_deemph(reinterpret_cast<float*>(V), audio, first, cnt, s);
    }

    // WBFM with every transform through rocFFT (lengths outside the engine, or RCFM_FFT=rocfft).
    void run_wbfm_rocfft(int first, int cnt, const float2* iq, float* audio, hipStream_t s, const float* theta) {
        size_t need = 0;
        FftPlan& fft_real_B = r2c_B.get(FftKind::R2C, B, cnt, false, need);
        FftPlan& ifft_B = c2c_inv_B.get(FftKind::C2C_INVERSE, B, cnt, true, need);
        FftPlan& fft_B = c2c_fwd_B.get(FftKind::C2C_FORWARD, B, cnt, true, need);
        FftPlan& ifft_A = c2c_inv_A.get(FftKind::C2C_INVERSE, A, cnt, true, need);
        work.reserve(need);
        pilot_stage(iq, theta, cnt, PilotBlocked{}, s);
        float* m = buf_m.as<float>();
        float* p = buf_p.as<float>();
        float2* P = buf_P.as<float2>();
        float2* Z = buf_Z.as<float2>();
        float2* V = buf_V.as<float2>();
        // wbfm.py:80 / pll.py:34  analytic signal of the pilot
        {
            StageTimer tm(ST_FFT_REAL_B, s);
            fft_real_B.exec(p, P, work.get(), s);
        }
        {
            StageTimer tm(ST_HILBERT_MASK, s);
            launch_hilbert_mask(P, Z, B, cnt, 1.0f / (float)B, s);
        }
        {
            StageTimer tm(ST_IFFT_B, s);
            ifft_B.exec(Z, Z, work.get(), s);
        }
        // wbfm.py:83,86-87  38 kHz carrier, L-R, stereo matrix; both legs packed in one complex signal
        {
            StageTimer tm(ST_STEREO_MIX, s);
            launch_stereo_mix(Z, m, Z, (size_t)cnt * B, s);
        }
        {
            StageTimer tm(ST_FFT_B, s);
            fft_B.exec(Z, Z, work.get(), s);
        }
        {
            StageTimer tm(ST_AUDIO_SPECTRUM, s);
            launch_stereo_unpack(Z, B, V, A, cnt, geom.wr.as<float>(), geom.nyq, geom.nyq_bin,
                                 geom.nyq_factor, geom.scale, nullptr, s);
        }
        {
            StageTimer tm(ST_IFFT_A, s);
            ifft_A.exec(V, V, work.get(), s);   // -> [cnt][A][2] float32, L/R interleaved
        }
        run_deemph(reinterpret_cast<float*>(V), audio, first, cnt, s, /*generic_fir=*/true);
    }

    // The FM / MFM routes below end at the decimated signal dst.
    // Two channels per complex signal from the pair FFT through the decimation to the inverse FFT:
    // 3 launches, no B-point spectrum in memory, half the inverse transforms
    void run_pair_decim(int cnt, float* dst, hipStream_t s, const float* theta, PhaseRows rows) {
        const bool nw = narrow(cnt);
        {
            StageTimer tm(ST_FFT_REAL_B, s);
            TILE_CALL(nw, fused_real_pair_fft_first, *eng_B, theta != nullptr ? theta : buf_m.as<float>(), buf_T.as<float2>(), cnt,
                      theta != nullptr, s, rows);
        }
        {
            StageTimer tm(ST_IFFT_A, s);
            TILE_CALL(nw, fused_fft_decim_ifft_pairs, *eng_B, *eng_Ad, buf_T.as<float2>(), dst, buf_TA.as<float2>(), cnt,
                      geom.wr.as<float>(), geom.scale, buf_dc.as<float2>(), s);
        }
    }

    // FM / MFM on the FFT engine without the decimating tile: pair FFT, a separate resampling kernel, real-output IFFT_A.
    void run_fm_engine(int cnt, float* dst, hipStream_t s, const float* theta, PhaseRows rows) {
        const bool nw = narrow(cnt);
        float* d = buf_m.as<float>();
        float2* Dfull = buf_Z.as<float2>();
        float2* Yfull = buf_V.as<float2>();
        {
            StageTimer tm(ST_FFT_REAL_B, s);
            // two channels per complex FFT; only |k| <= A/2 is kept (and read back by the unpacking).
            // From the tuner's phases the discriminator is the load of the first pass.
            if (theta != nullptr)
                TILE_CALL(nw, fused_real_pair_fft, *eng_B, theta, Dfull, buf_T.as<float2>(), cnt, std::min(A, B) / 2, s, true, rows);
            else
                TILE_CALL(nw, fused_real_pair_fft, *eng_B, d, Dfull, buf_T.as<float2>(), cnt, std::min(A, B) / 2, s);
        }
        {
            StageTimer tm(ST_AUDIO_SPECTRUM, s);
            launch_spectrum_real_full(Dfull, B, Yfull, A, cnt, geom.wr.as<float>(), geom.nyq, geom.nyq_bin,
                                      geom.nyq_factor, geom.scale, buf_dc.as<float2>(), true, s);
        }
        {
            StageTimer tm(ST_IFFT_A, s);
            TILE_CALL(nw, fused_ifft_real_out, *eng_A, Yfull, dst, buf_TA.as<float2>(), cnt, 1.0f, s);
        }
    }

    // FM / MFM with every transform through rocFFT.
    void run_fm_rocfft(int cnt, float* dst, hipStream_t s) {
        size_t need = 0;
        FftPlan& f1 = r2c_B.get(FftKind::R2C, B, cnt, false, need);
        FftPlan& f2 = c2r_A.get(FftKind::C2R, A, cnt, false, need);
        work.reserve(need);
        float2* D = buf_P.as<float2>();
        float2* Y = buf_V.as<float2>();
        {
            StageTimer tm(ST_FFT_REAL_B, s);
            f1.exec(buf_m.get(), D, work.get(), s);
        }
        {
            StageTimer tm(ST_AUDIO_SPECTRUM, s);
            launch_spectrum_r2c(D, B, Y, A, cnt, geom.wr.as<float>(), geom.nyq, geom.nyq_bin, geom.nyq_factor,
                                geom.scale, s);
        }
        StageTimer tm(ST_IFFT_A, s);
        f2.exec(Y, dst, work.get(), s);
    }

    // Narrow FM / MFM channels whose whole chain fits the LDS of a CU: gather, IFFT_B, discriminator, FFT_B,
    // decimation and IFFT_A of a channel pair in ONE kernel (lds_chain.h); only the audio reaches memory.
    void run_lds_chain(rcfm_tuner_s& t, int first, int cnt, float* audio, hipStream_t s) {
        t.require_readable(first, cnt, "rcfm_pipeline_run", RCFM_ERR_SIZE, "input_sig size and input_size mismatch");
        const ResampleGeom& tg = t.band(B).geom;
        // MFM: de-emphasis, mean removal and clip (mfm.py:62-66) run inside the same kernel when the taps are the
        // one-pole response deemphasis.py:37-46 designs (always, unless a caller replaced them): only the audio
        // leaves the chip.  Otherwise the chain stops at the decimated signal and the de-emphasis launches follow.
        const bool deemph_on_chip = kind == RCFM_MFM && opt_lds_deemph && deemph_geometric() &&
                                    lds_chain_deemph_supported(B, A);
        float* dst = (kind == RCFM_FM || deemph_on_chip) ? audio : buf_v.as<float>();
        LdsChainArgs a{t.spectrum(), t.base_dev.as<int32_t>() + first, t.n, tg.nyq,
                       tg.nyq_mode == NYQ_DOWN ? tg.nyq - 1 : -1, geom.wr.as<float>(), geom.scale, dst,
                       buf_dc.as<float2>(), cnt};
        if (deemph_on_chip) {
            a.deemph_taps = taps_sfx_dev();
            a.deemph_state = state_at(first);
            a.dc = nullptr;
        }
        {
            std::optional<StreamFence::Scope> fenced;   // the on-chip de-emphasis reads and writes the state
            if (deemph_on_chip) fenced.emplace(state_buf->fence, s);
            StageTimer tm(ST_LDS_CHAIN, s);
            RC_REQUIRE(launch_lds_chain(B, A, a, s), RCFM_ERR_RUNTIME, "LDS chain refused a geometry it lists");
        }
        if (kind == RCFM_MFM && !deemph_on_chip) run_deemph(dst, audio, first, cnt, s);
    }

    // RCFM_OPT_GRAPH for a one-channel call: replay the graph captured for these pointers, or capture one on the second
    // call in a row with them.  false: the caller launches the chain itself.
    bool run_graphed(int first, const float2* iq, float* audio, hipStream_t s) {
        if (!opt_graph || !eng_B || g_prof.mask != 0 || state_buf->fence.armed() || agc_on) return false;   // AGC: never captured
        const float* st = stateful() ? state_ptr() : nullptr;
        for (auto& g : graphs)
            if (g.iq == iq && g.audio == audio && g.first == first && g.state == st) {
                g.used = ++graph_tick;
                RC_HIP(hipGraphLaunch(g.exec, s));
                return true;
            }
        const auto& lc = last_call;
        if (lc.iq == iq && lc.audio == audio && lc.first == first && lc.state == st) {
            // second call in a row with these pointers: capture (on a stream of the handle's own) and replay
            if (!cap_stream) RC_HIP(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            bool ok = hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                try {
                    run_chunk(first, 1, iq, audio, cap_stream);
                } catch (...) {
                    ok = false;
                }
                if (hipStreamEndCapture(cap_stream, &graph) != hipSuccess || graph == nullptr) ok = false;
            }
            if (ok && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) ok = false;
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            if (ok) {
                if (graphs.size() >= 8) {   // a host that rotates more than eight buffer pairs: least recently used goes
                    size_t lru = 0;
                    for (size_t i = 1; i < graphs.size(); ++i)
                        if (graphs[i].used < graphs[lru].used) lru = i;
                    (void)hipGraphExecDestroy(graphs[lru].exec);
                    graphs.erase(graphs.begin() + (long)lru);
                }
                graphs.push_back(GraphSlot{iq, audio, st, first, exec, ++graph_tick});
                RC_HIP(hipGraphLaunch(exec, s));
                return true;
            }
            opt_graph = false;   // this runtime cannot capture the chain: plain launches from now on
        }
        last_call = GraphSlot{iq, audio, st, first, nullptr, 0};
        return false;
    }
};

extern "C" {

int rcfm_demod_create(int kind, int C, int B, int A, double tau, int chunk, rcfm_demod_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "out is NULL");
        RC_REQUIRE((kind >= RCFM_FM && kind <= RCFM_AM) || kind == RCFM_USB || kind == RCFM_LSB, RCFM_ERR_ARG,
                   "unknown demodulator kind");
        RC_REQUIRE(C >= 1 && B >= 2 && A >= 1, RCFM_ERR_ARG, "bad demodulator size");
        auto d = std::make_unique<rcfm_demod_s>();
        ArenaScope scope(d->arena);
        d->kind = kind;
        d->C = C;
        d->B = B;
        d->A = A;
        d->tau = tau;
        d->ch = (kind == RCFM_WBFM) ? 2 : 1;
        if (chunk <= 0) {
            // Measured on MI355X (profiles/r01_c_chunk_sweep.txt): bigger chunks keep winning -- the kernels are
            // tile-latency bound below ~64 channels per launch, and every launch pays one partial last wave of
            // workgroups: 1024 channels of 240 kHz per launch (9.8 GB of workspace) are 1.3 % faster than 512.
            // Narrow channels take proportionally more per launch (the same workspace): cfg5 (B = 12 500) measured
            // 2.23 / 2.10 / 2.06 / 2.05 ms at 1024 / 2048 / 4096 / 8192 channels per launch.
            chunk = (int)std::min<int64_t>(8192, std::max<int64_t>(1024, (int64_t)1024 * 240000 / B));
        }
        d->chunk = std::min(chunk, C);
        d->geom.build(B, A, 0.54 /* hamm */, false);
        std::memset(d->pilot_h, 0, sizeof(d->pilot_h));
        if (kind == RCFM_WBFM) {
            // wbfm.py:45-46: Bandpass(B, 19e3-50, 19e3+50, num_taps=41); cut-offs relative to Nyquist
            const double nyq = 0.5 * (double)B;
            const double lo = (19e3 - 50) / nyq, hi = (19e3 + 50) / nyq;
            RC_REQUIRE(hi < 1.0, RCFM_ERR_ARG, "Invalid cutoff frequency: frequencies must be greater than 0 and less than fs/2.");
            RC_REQUIRE(B > 3 * 41, RCFM_ERR_ARG, "The length of the input vector x must be greater than padlen, which is 123.");
            auto h = firwin_bandpass(41, lo, hi);
            for (int i = 0; i < 41; ++i) d->pilot_h[i] = (float)h[i];
            auto g = zero_phase_kernel(d->pilot_h, 41);
            std::memcpy(d->pilot_g_h, g.data(), sizeof(d->pilot_g_h));
            d->pilot_g.upload(g.data(), g.size() * sizeof(float));
            d->side_tap = (B % 2) ? (float)(0.23 * std::cos(kPi / (double)B)) : 0.23f;
        }
        if (d->stateful()) {
            deemphasis_design(A, tau, d->taps_h, d->zi_h);
            d->taps.upload(d->taps_h, sizeof(d->taps_h));
            d->state_buf->reset((size_t)C * d->ch * 50 * sizeof(float));
            d->reset_state(nullptr);
        }
        d->alloc();
        *out = d.release();
    });
}

int rcfm_demod_run(rcfm_demod_t d, int first, int count, const void* iq, void* audio, void* stream) {
    return guarded([&] {
        RC_REQUIRE(d && iq && audio, RCFM_ERR_ARG, "NULL argument");
        require_channels(first, count, d->C);
        ArenaScope scope(d->arena);
        const float2* in = static_cast<const float2*>(iq);
        float* outp = static_cast<float*>(audio);
        if (count == 1 && d->run_graphed(first, in, outp, as_stream(stream))) return;
        for (int off = 0; off < count; off += d->chunk) {
            const int cnt = std::min(d->chunk, count - off);
            d->run_chunk(first + off, cnt, in + (size_t)off * d->B, outp + (size_t)off * d->A * d->ch,
                         as_stream(stream));
        }
    });
}

int rcfm_demod_reset_state(rcfm_demod_t d, void* stream) {
    return guarded([&] {
        RC_REQUIRE(d, RCFM_ERR_ARG, "NULL handle");
        d->reset_state(as_stream(stream));
    });
}

int rcfm_demod_get_state(rcfm_demod_t d, float* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(d && state_host, RCFM_ERR_ARG, "NULL argument");
        if (!d->stateful()) return;
        state_to_host(state_host, d->state_ptr(), (size_t)d->C * d->ch * 50 * sizeof(float), as_stream(stream));
    });
}

int rcfm_demod_set_state(rcfm_demod_t d, const float* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(d && state_host, RCFM_ERR_ARG, "NULL argument");
        if (!d->stateful()) return;
        state_to_device(d->state_ptr(), state_host, (size_t)d->C * d->ch * 50 * sizeof(float), as_stream(stream));
    });
}

int rcfm_demod_bind_state(rcfm_demod_t single, rcfm_demod_t batched, int index, int move_history, void* stream) {
    return guarded([&] {
        RC_REQUIRE(single && batched, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(single != batched && single->kind == batched->kind && single->A == batched->A &&
                       single->tau == batched->tau,
                   RCFM_ERR_ARG, "bind_state needs demodulators of one class, audio rate and time constant");
        RC_REQUIRE(single->agc_on == batched->agc_on &&
                       (!single->agc_on || (single->agc_decay == batched->agc_decay && single->agc_level == batched->agc_level &&
                                            single->agc_floor == batched->agc_floor)),
                   RCFM_ERR_ARG, "bind_state needs equal AGC settings on both demodulators");
        require_channels(index, single->C, batched->C);
        if (!single->carries_state()) return;   // fm.py carries no state, nor do AM, USB and LSB without AGC
        const size_t per = (size_t)single->C * single->state_stride();
        const size_t slot = batched->state_off + (size_t)index * single->state_stride();
        float* dst = batched->state_at(index);
        if (single->state_buf == batched->state_buf && single->state_off == slot) return;   // already bound to this slot
        if (move_history) {
            // the history this demodulator has carried so far moves into the slot (stream-ordered)
            RC_HIP(hipMemcpyAsync(dst, single->state_ptr(), per * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
            RC_HIP(hipStreamSynchronize(as_stream(stream)));   // the old buffer may be freed right below
        }
        single->drop_graphs();
        single->state_buf = batched->state_buf;
        single->state_off = slot;
    });
}

int rcfm_demod_set_option(rcfm_demod_t d, int option, int value) {
    return guarded([&] {
        RC_REQUIRE(d, RCFM_ERR_ARG, "NULL handle");
        d->drop_graphs();
        switch (option) {
            case RCFM_OPT_GRAPH: d->opt_graph = value != 0; break;
            case RCFM_OPT_LDS_CHAIN: d->opt_lds_chain = value != 0; break;
            case RCFM_OPT_FUSED_TILES: d->opt_pilot_chain = d->opt_decim_tile = value != 0; break;
            case RCFM_OPT_PILOT_CHAIN: d->opt_pilot_chain = value != 0; break;
            case RCFM_OPT_DECIM_TILE: d->opt_decim_tile = value != 0; break;
            case RCFM_OPT_PILOT_BLOCKED: d->opt_pilot_blocked = value != 0; break;
            case RCFM_OPT_LDS_DEEMPH: d->opt_lds_deemph = value != 0; break;
            case RCFM_OPT_PHASE_LINK: d->opt_phase_link = value != 0; break;
            case RCFM_OPT_SSB_DIRECT: d->opt_ssb_direct = value != 0; break;
            case RCFM_OPT_NARROW_TILES:
                RC_REQUIRE(value >= 0 && value <= 2, RCFM_ERR_ARG, "narrow tiles: 0 never, 1 automatic, 2 always");
                d->opt_narrow = value;
                break;
            case RCFM_OPT_STATE_FENCE: d->state_buf->fence.arm(value != 0); break;
            default: RC_REQUIRE(false, RCFM_ERR_ARG, "unknown demodulator option");
        }
    });
}

int rcfm_demod_get_option(rcfm_demod_t d, int option, int* value) {
    return guarded([&] {
        RC_REQUIRE(d && value, RCFM_ERR_ARG, "NULL handle or output");
        switch (option) {
            case RCFM_OPT_LDS_CHAIN: *value = d->opt_lds_chain; break;
            case RCFM_OPT_FUSED_TILES: *value = d->opt_pilot_chain && d->opt_decim_tile; break;
            case RCFM_OPT_PILOT_CHAIN: *value = d->opt_pilot_chain; break;
            case RCFM_OPT_DECIM_TILE: *value = d->opt_decim_tile; break;
            // the EFFECTIVE value: the switch is on and this handle's geometry has the layout (and the chain that reads it)
            case RCFM_OPT_PILOT_BLOCKED:
                *value = d->opt_pilot_blocked && d->opt_pilot_chain && d->pilot_blocked().valid() &&
                         fused_pilot_chain_applies(*d->eng_B, *d->eng_Bi, 2);
                break;
            case RCFM_OPT_LDS_DEEMPH: *value = d->opt_lds_deemph; break;
            case RCFM_OPT_PHASE_LINK: *value = d->opt_phase_link; break;
            case RCFM_OPT_SSB_DIRECT: *value = d->opt_ssb_direct; break;
            case RCFM_OPT_NARROW_TILES: *value = d->opt_narrow; break;
            case RCFM_OPT_STATE_FENCE: *value = d->state_buf->fence.armed(); break;
            // 0 = off (or this runtime refused the capture), 1 = on, 1 + k = on and k captured chains are being replayed
            case RCFM_OPT_GRAPH: *value = d->opt_graph ? 1 + (int)d->graphs.size() : 0; break;
            default: RC_REQUIRE(false, RCFM_ERR_ARG, "unknown demodulator option");
        }
    });
}

int rcfm_demod_set_agc(rcfm_demod_t d, double decay_samples, float level, float floor) {
    return guarded([&] {
        RC_REQUIRE(d, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(d->kind == RCFM_AM || d->ssb(), RCFM_ERR_ARG, "AGC is for AM, USB and LSB demodulators");
        RC_REQUIRE(std::isfinite(decay_samples) && decay_samples >= 0.0, RCFM_ERR_ARG, "AGC decay_samples must be finite and >= 0");
        if (decay_samples == 0.0) {   // off again: the per-buffer normalisation
            d->agc_on = false;
            return;
        }
        RC_REQUIRE(std::isfinite(level) && level > 0.f, RCFM_ERR_ARG, "AGC level must be finite and > 0");
        RC_REQUIRE(std::isfinite(floor) && floor >= 0.f, RCFM_ERR_ARG, "AGC floor must be finite and >= 0");
        // a state of this handle's own (a fence armed on a shared one stays with the others)
        d->state_buf = std::make_shared<rcfm_demod_s::StateBuf>();
        d->state_buf->reset((size_t)d->C * sizeof(float));
        d->state_off = 0;
        d->agc_on = true;
        d->agc_decay = decay_samples;
        d->agc_level = level;
        d->agc_floor = floor;
        d->reset_state(nullptr);
    });
}

int rcfm_demod_get_agc_state(rcfm_demod_t d, float* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(d && state_host, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(d->agc_on, RCFM_ERR_STATE, "this demodulator has no AGC (rcfm_demod_set_agc)");
        state_to_host(state_host, d->state_ptr(), (size_t)d->C * sizeof(float), as_stream(stream));
    });
}

int rcfm_demod_set_agc_state(rcfm_demod_t d, const float* state_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(d && state_host, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(d->agc_on, RCFM_ERR_STATE, "this demodulator has no AGC (rcfm_demod_set_agc)");
        state_to_device(d->state_ptr(), state_host, (size_t)d->C * sizeof(float), as_stream(stream));
    });
}

int rcfm_demod_get_taps(rcfm_demod_t d, float* deemph51_host, float* pilot41_host) {
    return guarded([&] {
        RC_REQUIRE(d, RCFM_ERR_ARG, "NULL handle");
        if (deemph51_host) std::memcpy(deemph51_host, d->taps_h, sizeof(d->taps_h));
        if (pilot41_host) std::memcpy(pilot41_host, d->pilot_h, sizeof(d->pilot_h));
    });
}

int rcfm_demod_destroy(rcfm_demod_t d) {
    return guarded([&] { delete d; });
}


int rcfm_pipeline_run(rcfm_tuner_t t, rcfm_demod_t d, int first, int count, void* audio, void* stream) {
    return guarded([&] {
        RC_REQUIRE(t && d && audio, RCFM_ERR_ARG, "NULL argument");
        require_channels(first, count, std::min(t->nch, d->C));
        ArenaScope scope(d->arena);
        hipStream_t s = as_stream(stream);
        d->buf_iq.reserve((size_t)d->chunk * d->B * sizeof(float2));
        for (int off = 0; off < count; off += d->chunk) {
            const int c0 = first + off, cnt = std::min(d->chunk, count - off);
            float* out_c = static_cast<float*>(audio) + (size_t)off * d->A * d->ch;
            RC_REQUIRE(t->bw[c0] == d->B, RCFM_ERR_SIZE, "input_sig size and input_size mismatch");
            // RCFM_OPT_LDS_CHAIN = 0: the multi-pass launches.  The chain computes the FM discriminator: FM / MFM only.
            if (d->opt_lds_chain && (d->kind == RCFM_FM || d->kind == RCFM_MFM) && lds_chain_supported(d->B, d->A) &&
                t->fast_gather_ok(c0)) {
                d->run_lds_chain(*t, c0, cnt, out_c, s);
                continue;
            }
            // USB / LSB: everything is linear and the wideband spectrum is already loaded -- no channel samples at all.
            // RCFM_OPT_SSB_DIRECT = 0 (or a geometry the fast gather refuses): complex hand-over + route 2 below.
            if (d->ssb_direct_ok(*t, c0)) {
                d->run_ssb_direct(*t, c0, cnt, out_c, s);
                continue;
            }
            // AM's counterpart of the phase link: the tuner's last pass stores |x| (float32, contiguous) straight into
            // the buffer the envelope kernel would fill.  RCFM_OPT_PHASE_LINK = 0: complex hand-over + envelope kernel.
            if (d->kind == RCFM_AM && d->opt_phase_link && t->phase_capable(c0)) {
                {
                    ArenaScope ts(t->arena);
                    t->run(c0, cnt, nullptr, s, d->buf_m.as<float>(), 0, d->opt_narrow, /*envelope=*/true);
                }
                d->run_am(c0, cnt, nullptr, out_c, s, /*envelope_ready=*/true);
                continue;
            }
            // Every demodulator starts with the FM discriminator, which only needs the samples' phases:
            // the tuner's last pass leaves angle(x) / pi (float32) instead of x (complex64) -- half the
            // bytes written here and read back by the first demod kernel.  RCFM_OPT_PHASE_LINK = 0: complex hand-over.
            if (d->opt_phase_link && d->phase_capable() && t->phase_capable(c0)) {
                // FM / MFM read the phases through LoadPhaseStepPair, which understands padded rows: when the tuner's
                // last pass would store rows of n_1 phases that are not whole 64-byte segments apart (cfg5: n_1 = 100),
                // the rows go to a pitch of whole 128-byte lines.  (WBFM's pilot stage reads contiguous phases.)
                PhaseRows rows;
                const int n1 = t->band_row_length(c0);
                if (d->kind != RCFM_WBFM && d->eng_B && t->band_two_pass(c0) && n1 > 0 &&
                    n1 % 16 != 0 && d->B % n1 == 0 && d->B < (1 << 20) && n1 < (1 << 12)) {
                    rows.row = n1;
                    rows.pitch = (n1 + 15) / 16 * 16;     // floats: a 64-byte store segment never straddles a line
                    d->buf_iq.reserve((size_t)d->chunk * rows.channel_stride(d->B) * sizeof(float));
                }
                float* theta = d->buf_iq.as<float>();
                {
                    ArenaScope ts(t->arena);
                    t->run(c0, cnt, nullptr, s, theta, rows.pitch, d->opt_narrow);
                }
                d->run_chunk(c0, cnt, nullptr, out_c, s, theta, rows);
                continue;
            }
            {
                ArenaScope ts(t->arena);
                t->run(c0, cnt, d->buf_iq.as<float2>(), s, nullptr, 0, d->opt_narrow);
            }
            d->run_chunk(c0, cnt, d->buf_iq.as<float2>(), out_c, s);
        }
    });
}

}  // extern "C"
