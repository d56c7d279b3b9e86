// The tuner handle (rcfm_tuner_*): the wideband forward FFT of a buffer, then each channel's bins gathered, weighted
// and transformed back at the channel's bandwidth.

#include "api_internal.h"

#include <cmath>

using namespace rcfm;

// Rows of the spectrum (row = n_1 consecutive bins, n_1 = the forward plan's first pass length) that channels
// [first, first + count) read, as a circular window lo..hi: everything but the longest run of unused rows.
// false: no engine, too few rows, or nothing worth skipping -- the range reads (nearly) the whole spectrum.
bool rcfm_tuner_s::row_window(int first, int count, FftRowWindow* w, const FftEngine* eng) const {
    if (!eng) eng = forward_engine.get();
    if (!eng || count == 0) return false;
    const int64_t f0 = eng->row_length();
    const int64_t rows = n / f0;
    if (rows < 64) return false;
    std::vector<char> used((size_t)rows, 0);
    for (int c = first; c < first + count; ++c) {
        const int64_t centre = (n - roll[c]) % n, h = bw[c] / 2 + 2;
        const int64_t r0 = (centre - h) / f0 - ((centre - h) < 0 ? 1 : 0), r1 = (centre + h) / f0;
        for (int64_t r = r0; r <= r1; ++r) used[(size_t)(((r % rows) + rows) % rows)] = 1;
    }
    // the longest circular run of unused rows is dropped; everything else is kept
    int64_t best_len = 0, best_start = 0, run = 0;
    for (int64_t i = 0; i < 2 * rows; ++i) {
        if (!used[(size_t)(i % rows)]) {
            ++run;
            if (run > best_len && run <= rows) {
                best_len = run;
                best_start = i - run + 1;
            }
        } else {
            run = 0;
        }
    }
    if (best_len < rows / 64 || best_len >= rows) return false;   // nothing worth skipping (or nothing used)
    w->lo = (int)((best_start + best_len) % rows);
    w->hi = (int)(((best_start - 1) % rows + rows) % rows);
    return true;
}

void rcfm_tuner_s::shard(int first, int count) {
    require_channels(first, count, nch);
    shard_first = first;
    shard_count = count;
    windowed = row_window(first, count, &window);
    windowed_aligned = forward_aligned && row_window(first, count, &window_aligned, forward_aligned.get());
}

// The same window in bins: [first_bin, first_bin + nbins) modulo n (nbins = n: everything).
void rcfm_tuner_s::bin_window(int first, int count, int64_t* first_bin, int64_t* nbins) const {
    FftRowWindow w{0, 0};
    if (count == 0) {            // a rank that owns no channels (C < G) reads nothing
        *first_bin = 0;
        *nbins = 0;
        return;
    }
    if (!row_window(first, count, &w)) {
        *first_bin = 0;
        *nbins = n;
        return;
    }
    const int64_t f0 = forward_engine->row_length(), rows = n / f0;
    *first_bin = (int64_t)w.lo * f0;
    *nbins = (((int64_t)w.hi - w.lo + rows) % rows + 1) * f0;
}

// The caller has written the bins channels [first, first + count) read (bin_window) into the spectrum storage,
// e.g. received them from the GPU that ran the wideband FFT of this buffer: repeat the ends in the halos
// (what the last FFT pass does for a local load) and accept exactly that channel range.
void rcfm_tuner_s::adopt(int first, int count, hipStream_t s) {
    require_channels(first, count, nch);
    int64_t fb = 0, nb = 0;
    bin_window(first, count, &fb, &nb);
    RC_REQUIRE(!ext_window || (first == ext_first && count == ext_count), RCFM_ERR_STATE,
               "the attached storage holds the window of another channel range (rcfm_tuner_attach_window)");
    if (halo > 0 && !ext_window) {
        float2* Xs = spectrum();
        // segments of the window: [fb, min(fb + nb, n)) and, when it wraps, [0, fb + nb - n)
        const int64_t seg[2][2] = {{fb, std::min(fb + nb, n)}, {0, fb + nb > n ? fb + nb - n : 0}};
        for (auto& g : seg) {
            const int64_t a0 = std::max<int64_t>(g[0], 0), a1 = std::min<int64_t>(g[1], halo);   // bins [0, halo) -> behind the end
            if (a1 > a0)
                RC_HIP(hipMemcpyAsync(Xs + n + a0, Xs + a0, sizeof(float2) * (size_t)(a1 - a0), hipMemcpyDeviceToDevice, s));
            const int64_t b0 = std::max<int64_t>(g[0], n - halo), b1 = std::min<int64_t>(g[1], n);     // bins [n - halo, n) -> in front
            if (b1 > b0)
                RC_HIP(hipMemcpyAsync(Xs + (b0 - n), Xs + b0, sizeof(float2) * (size_t)(b1 - b0), hipMemcpyDeviceToDevice, s));
        }
    }
    set_loaded(true, nb < n, first, count);
    set_held(fb, nb);
}

// The bins [fb, fb + nb) of channels [first, first + count), which must be able to live in a storage of their own,
// [halo | nb | halo]: a window that neither wraps around bin 0 nor touches the far ends (whose halos repeat the other
// end of the spectrum).
void rcfm_tuner_s::window_storage(int first, int count, int64_t* fb, int64_t* nb) const {
    require_channels(first, count, nch);
    bool ok = halo > 0 && count > 0;
    if (ok) {
        bin_window(first, count, fb, nb);
        ok = *nb < n && *fb >= halo && *fb + *nb <= n - halo;
    }
    RC_REQUIRE(ok, RCFM_ERR_SIZE,
               "these channels' bins wrap around the ends of the spectrum (or are all of it): no window storage");
}

rcfm_tuner_s::Band& rcfm_tuner_s::band(int32_t b) {
    auto it = bands.find(b);
    if (it == bands.end()) {
        auto nb = std::make_unique<Band>();
        nb->geom.build(n, b, 0.5 /* hann */, true);
        FftPlanDesc probe;
        if (use_engine() && fft_plan_describe(b, &probe)) nb->engine = std::make_unique<FftEngine>(b);
        it = bands.emplace(b, std::move(nb)).first;
    }
    return *it->second;
}

// The fast gather's preconditions (fused_passes.hip, LoadTunerGatherFast) for the band of channel `first`: haloed
// spectrum with 32-bit bases, window argument small enough for the series, no up-sampling Nyquist rule.
bool rcfm_tuner_s::fast_gather_ok(int first) {
    if (first < 0 || first >= nch || halo <= 0) return false;
    const int32_t B = bw[first];
    const ResampleGeom& g = band(B).geom;
    const bool series = 6.28318530717958647692 * ((double)(B / 2 + 2) / (double)n) < 0.25;
    return series && halo >= B / 2 + 1 && g.nyq_mode != NYQ_UP && B <= n;
}

// The same preconditions for reading a channel of bandwidth B as one run of the haloed spectrum (levels()); no band is
// built for it.  (B <= n always holds here, so the Nyquist rule is never the up-sampling one.)
bool rcfm_tuner_s::fast_bins_ok(int32_t B) const {
    const bool series = 6.28318530717958647692 * ((double)(B / 2 + 2) / (double)n) < 0.25;
    return halo > 0 && series && halo >= B / 2 + 1 && B <= n;
}

// The B bins d = -(B / 2) .. of a channel as one run of the haloed spectrum, unweighted (carriers()): the halo reaches
// them, nothing more -- no window is evaluated, so the series precondition of fast_bins_ok does not apply.
bool rcfm_tuner_s::halo_run_ok(int32_t B) const { return halo > 0 && halo >= B / 2 + 1 && B <= n; }

// Can run() leave angle(x) / pi instead of x for this channel's band?  (engine path only)
bool rcfm_tuner_s::phase_capable(int first) { return first >= 0 && first < nch && band(bw[first]).engine != nullptr; }

// First pass length n_1 of the band's inverse FFT (0 without an engine): its last pass stores rows of n_1 samples.
int rcfm_tuner_s::band_row_length(int first) { return phase_capable(first) ? (int)band(bw[first]).engine->row_length() : 0; }

// Padded phase rows (fused_tuner_ifft's theta_pitch) need the last pass to write rows of n_1 samples with no
// outer line index, i.e. a TWO-pass plan (B <= 262144); three-pass bands keep contiguous phases.
bool rcfm_tuner_s::band_two_pass(int first) { return phase_capable(first) && band(bw[first]).engine->npass() == 2; }

// Channels [first, first + count) may be read from the loaded spectrum: it was loaded, for a shard and into a storage
// that hold them.  `caller` names the entry point in the error.
void rcfm_tuner_s::require_loaded(int first, int count, const char* caller) const {
    RC_REQUIRE(loaded, RCFM_ERR_STATE, std::string(caller) + " called before rcfm_tuner_load");
    RC_REQUIRE(!loaded_windowed || (first >= loaded_first && first + count <= loaded_first + loaded_count),
               RCFM_ERR_STATE,
               "channel outside the shard the spectrum was loaded for (rcfm_tuner_shard, then rcfm_tuner_load)");
    RC_REQUIRE(!ext_window || (first >= ext_first && first + count <= ext_first + ext_count), RCFM_ERR_STATE,
               "channel outside the window the attached storage holds (rcfm_tuner_attach_window)");
}

// ... and they share one bandwidth (else bw_code / bw_msg).
void rcfm_tuner_s::require_readable(int first, int count, const char* caller, int bw_code, const char* bw_msg) const {
    require_loaded(first, count, caller);
    for (int i = 0; i < count; ++i) RC_REQUIRE(bw[first + i] == bw[first], bw_code, bw_msg);
}

// power[i] = the level of channel first + i (include/rcfm.h, rcfm_tuner_levels): one read of the channel's bins.  The
// fast form needs every channel of the range to pass fast_bins_ok; the number of workgroups a channel is split over
// depends on its bandwidth alone (level_segments), so the sums have one order on every device and stream.
void rcfm_tuner_s::levels(int first, int count, float* power, hipStream_t s) {
    require_channels(first, count, nch);
    require_loaded(first, count, "rcfm_tuner_levels");
    if (count == 0) return;
    bool fast = true;
    int segs = 1;
    for (int c = first; c < first + count; ++c) {
        RC_REQUIRE(bw[c] <= n, RCFM_ERR_ARG, "channel bandwidth exceeds the input bandwidth");
        fast = fast && fast_bins_ok(bw[c]);
        segs = std::max(segs, level_segments(bw[c]));
    }
    if (segs > 1) levels_part.reserve(sizeof(double) * (size_t)count * segs);
    StageTimer tm(ST_LEVELS, s);
    launch_channel_levels(spectrum(), n, fast ? base_dev.as<int32_t>() + first : nullptr, roll_dev.as<int64_t>() + first,
                          bw_dev.as<int32_t>() + first, count, segs, segs > 1 ? levels_part.as<double>() : nullptr, power, s);
}

// The carrier estimates of channels [first, first + count) (include/rcfm.h, rcfm_tuner_carriers; the arguments are checked
// there): one read of each channel's bins, unweighted.  The fast form needs every channel of the range to pass
// halo_run_ok; segments and their order as levels().  gate_n2 = gate n^2, the gate in units of |X|^2.
void rcfm_tuner_s::carriers(int first, int count, double gate_n2, int32_t* peak_bin, float* peak_power, float* centroid,
                            float* spread, hipStream_t s) {
    require_channels(first, count, nch);
    require_loaded(first, count, "rcfm_tuner_carriers");
    if (count == 0) return;
    bool fast = true;
    int segs = 1;
    for (int c = first; c < first + count; ++c) {
        RC_REQUIRE(bw[c] <= n, RCFM_ERR_ARG, "channel bandwidth exceeds the input bandwidth");
        fast = fast && halo_run_ok(bw[c]);
        segs = std::max(segs, level_segments(bw[c]));
    }
    if (segs > 1) carriers_part.reserve(sizeof(CarrierPart) * (size_t)count * segs);
    launch_channel_carriers(spectrum(), n, fast ? base_dev.as<int32_t>() + first : nullptr, roll_dev.as<int64_t>() + first,
                            bw_dev.as<int32_t>() + first, count, segs, gate_n2,
                            segs > 1 ? carriers_part.as<CarrierPart>() : nullptr, peak_bin, peak_power, centroid, spread, s);
}

// New rolls for channels [first, first + count) (include/rcfm.h, rcfm_tuner_retune).  The tables travel through pinned
// staging memory of the handle, so the caller's array is free at once and the copies are plain stream work.
void rcfm_tuner_s::retune(int first, int count, const int64_t* roll_host, hipStream_t s) {
    require_channels(first, count, nch);
    RC_REQUIRE(!ext_window, RCFM_ERR_STATE,
               "a window is attached: its layout was computed from the old rolls (rcfm_tuner_attach_window)");
    if (count == 0) return;
    const size_t roll_bytes = sizeof(int64_t) * (size_t)count, base_bytes = halo > 0 ? sizeof(int32_t) * (size_t)count : 0;
    if (stage_done) RC_HIP(hipEventSynchronize(stage_done));   // the previous retune's copies have read the staging memory
    else RC_HIP(hipEventCreateWithFlags(&stage_done, hipEventDisableTiming));
    if (stage_bytes < roll_bytes + base_bytes) {
        if (stage) RC_HIP(hipHostFree(stage));
        stage = nullptr;
        stage_bytes = 0;
        RC_HIP(hipHostMalloc(&stage, roll_bytes + base_bytes, hipHostMallocDefault));
        stage_bytes = roll_bytes + base_bytes;
    }
    int64_t* roll_stage = static_cast<int64_t*>(stage);
    int32_t* base_stage = reinterpret_cast<int32_t*>(roll_stage + count);
    for (int i = 0; i < count; ++i) {
        int64_t r = roll_host[i] % n;
        if (r < 0) r += n;
        roll[first + i] = roll_stage[i] = r;
        if (halo > 0) base_stage[i] = (int32_t)((n - r) % n);
    }
    RC_HIP(hipMemcpyAsync(roll_dev.as<int64_t>() + first, roll_stage, roll_bytes, hipMemcpyHostToDevice, s));
    if (halo > 0) RC_HIP(hipMemcpyAsync(base_dev.as<int32_t>() + first, base_stage, base_bytes, hipMemcpyHostToDevice, s));
    RC_HIP(hipEventRecord(stage_done, s));
    // the rows a sharded load keeps follow the rolls; a storage that holds a window only holds it for the old ones
    if (shard_count > 0) shard(shard_first, shard_count);
    if (loaded && (loaded_windowed || held_bins < n)) set_loaded(false, false, loaded_first, 0);
}

// power[m], peak[m] of cell m of the span [s0, s0 + L) of signed bins cut into M cells (include/rcfm.h,
// rcfm_tuner_power_spectrum; the arguments are checked there).  Every bin of the span must be held: the span is one run of
// elements, or two where it crosses signed bin 0, each inside [held_first, held_first + held_bins) modulo n.
void rcfm_tuner_s::power_spectrum(int64_t s0, int64_t L, int64_t M, float* power, float* peak, hipStream_t s) {
    RC_REQUIRE(loaded, RCFM_ERR_STATE, "rcfm_tuner_power_spectrum called before rcfm_tuner_load");
    const int64_t z = std::min(std::max<int64_t>(-s0, 0), L);   // span positions [0, z) are signed bins < 0
    const int64_t run[2][2] = {{s0 + n, z}, {s0 + z, L - z}};    // first element, length
    for (auto& r : run) {
        if (r[1] <= 0 || held_bins >= n) continue;
        const int64_t off = ((r[0] - held_first) % n + n) % n;
        RC_REQUIRE(off + r[1] <= held_bins, RCFM_ERR_STATE,
                   "the span reaches bins the loaded, sharded or attached spectrum does not hold (rcfm_tuner_window)");
    }
    const int segs = power_segments(L, M);
    if (segs > 1) {
        power_part_sum.reserve(sizeof(double) * (size_t)M * segs);
        power_part_max.reserve(sizeof(float) * (size_t)M * segs);
    }
    launch_power_spectrum(spectrum(), n, s0, L, M, segs > 1 ? power_part_sum.as<double>() : nullptr,
                          segs > 1 ? power_part_max.as<float>() : nullptr, power, peak, s);
}

// theta != nullptr (phase_capable bands only): angle(x) / pi goes to theta [count][B] float32, out is unused;
// envelope: |x| instead (AM).
void rcfm_tuner_s::run(int first, int count, float2* out, hipStream_t s, float* theta, int theta_pitch,
                       int narrow_mode, bool envelope) {
    if (narrow_mode < 0) narrow_mode = opt_narrow;
    require_channels(first, count, nch);
    require_readable(first, count, "rcfm_tuner_run", RCFM_ERR_ARG, "channels of one rcfm_tuner_run range must share a bandwidth");
    if (count == 0) return;
    const int32_t B = bw[first];
    Band& bd = band(B);
    const ResampleGeom& g = bd.geom;
    if (bd.engine) {
        // gather + window ride on the first pass of the inverse FFT (fused_passes.h)
        band_tmp.reserve((size_t)count * bd.engine->tmp_stride() * sizeof(float2));
        TunerGather tg{spectrum(), n, roll_dev.as<int64_t>() + first, 0.5, g.nyq, g.nneg, g.nyq_mode,
                       halo ? base_dev.as<int32_t>() + first : nullptr, halo};
        StageTimer tm(ST_TUNER_IFFT, s);
        TILE_CALL(narrow_launch(*bd.engine, count, narrow_mode), fused_tuner_ifft, *bd.engine, tg, out, band_tmp.as<float2>(), count, s,
                  theta, theta_pitch, envelope);
        return;
    }
    RC_REQUIRE(theta == nullptr, RCFM_ERR_STATE, "phase output needs the FFT engine");
    size_t need = 0;
    FftPlan& inv = bd.inverse.get(FftKind::C2C_INVERSE, (size_t)B, count, true, need);
    work.reserve(need);
    {
        StageTimer tm(ST_TUNER_GATHER, s);
        launch_spectrum_c2c(spectrum(), 0, n, roll_dev.as<int64_t>() + first, out, B, count,
                            g.wpos.as<float>(), g.wneg.as<float>(), g.w_merge, g.nyq, g.nneg, g.nyq_mode,
                            g.scale, s);
    }
    {
        StageTimer tm(ST_TUNER_IFFT, s);
        inv.exec(out, out, work.get(), s);
    }
}

extern "C" {

// ---- tuner -----------------------------------------------------------------

int rcfm_tuner_create(int64_t n, int nch, const int64_t* roll_host, const int32_t* bw_host, rcfm_tuner_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "out is NULL");
        RC_REQUIRE(n >= 1 && nch >= 0, RCFM_ERR_ARG, "bad tuner size");
        RC_REQUIRE(nch == 0 || (roll_host && bw_host), RCFM_ERR_ARG, "roll/bw is NULL");
        auto t = std::make_unique<rcfm_tuner_s>();
        ArenaScope scope(t->arena);
        t->n = n;
        t->nch = nch;
        t->roll.resize(nch);
        t->bw.assign(bw_host, bw_host + nch);
        for (int i = 0; i < nch; ++i) {
            RC_REQUIRE(bw_host[i] >= 1, RCFM_ERR_ARG, "channel bandwidth must be >= 1");
            // scipy.signal.resample(domain="freq") also up-samples; the Tuner never does
            RC_REQUIRE(bw_host[i] <= n, RCFM_ERR_ARG, "channel bandwidth exceeds the input bandwidth");
            int64_t r = roll_host[i] % n;
            if (r < 0) r += n;
            t->roll[i] = r;
        }
        if (nch) t->roll_dev.upload(t->roll.data(), sizeof(int64_t) * nch);
        if (nch) t->bw_dev.upload(t->bw.data(), sizeof(int32_t) * nch);
        // halo: whole 128-byte lines on both sides, wide enough for the widest channel -- and no wider than n / 2, so
        // that no bin belongs to both halos (FftRowWindow).  A handle with a channel wider than that keeps none: such a
        // channel never takes a form that reads the halos (fast_gather_ok, fast_bins_ok).
        int64_t h = 0;
        for (int i = 0; i < nch; ++i) h = std::max<int64_t>(h, bw_host[i] / 2 + 2);
        h = (h + 15) / 16 * 16;
        if (nch && 2 * h <= n && n + h < ((int64_t)1 << 31)) {
            t->halo = h;
            std::vector<int32_t> base(nch);
            for (int i = 0; i < nch; ++i) base[i] = (int32_t)((n - t->roll[i]) % n);
            t->base_dev.upload(base.data(), sizeof(int32_t) * nch);
        }
        FftPlanDesc probe;
        if (use_engine() && fft_plan_describe(n, &probe)) {
            t->forward_engine = std::make_unique<FftEngine>(n);
            int64_t tmp_elems = t->forward_engine->tmp_stride();
            int64_t order[3];
            if (fft_plan_aligned_order(t->forward_engine->desc(), order)) {
                t->forward_aligned = std::make_unique<FftEngine>(n, order, 3, 2);
                tmp_elems = std::max(tmp_elems, t->forward_aligned->tmp_stride());
            }
            t->forward_tmp.reset(sizeof(float2) * (size_t)tmp_elems);
        }
        t->X.reset(t->own_spectrum_bytes());
        if (!t->forward_engine) {
            t->forward = std::make_unique<FftPlan>(FftKind::C2C_FORWARD, (size_t)n, 1, false);
            t->forward_work.reserve(t->forward->work_bytes());
        }
        *out = t.release();
    });
}

// rcfm_tuner_load (format 0: x holds complex64) and rcfm_tuner_load_raw (RCFM_IQ_*: x holds integer pairs).
static int tuner_load(rcfm_tuner_t t, int format, const void* x, void* stream) {
    return guarded([&] {
        RC_REQUIRE(format == 0 || iq_format_ok(format), RCFM_ERR_ARG,
                   "unknown IQ format (RCFM_IQ_CS16, RCFM_IQ_CS8, RCFM_IQ_CU8)");
        RC_REQUIRE(t && x, RCFM_ERR_ARG, "NULL argument");
        // (the first pass loads a pair as one 4- or 2-byte word)
        RC_REQUIRE(format == 0 || !t->raw_fused() || (uintptr_t)x % (format == RCFM_IQ_CS16 ? 4 : 2) == 0, RCFM_ERR_ARG,
                   "misaligned buffer: rcfm_tuner_load_raw reads whole I, Q pairs");
        ArenaScope scope(t->arena);
        RC_REQUIRE(!t->ext_window, RCFM_ERR_STATE,
                   "rcfm_tuner_load needs storage for the whole spectrum: a window is attached (rcfm_tuner_attach_window)");
        RC_REQUIRE(t->iq_mode == RCFM_IQ_BALANCE_OFF ||
                       !(t->forward_engine && (t->use_aligned() ? t->windowed_aligned : t->windowed)),
                   RCFM_ERR_STATE,
                   "a sharded load keeps a window of the spectrum, the IQ balance needs every bin and its mirror "
                   "(rcfm_tuner_shard, rcfm_tuner_set_iq_balance)");
        {
            StageTimer tm(ST_TUNER_FFT, as_stream(stream));
            if (format != 0 && !t->raw_fused()) {   // no first pass to ride on: convert, then the complex64 load
                t->raw_c64.reserve(sizeof(float2) * (size_t)t->n);
                launch_iq_convert(format, (size_t)t->n, x, t->raw_c64.as<float2>(), as_stream(stream));
                x = t->raw_c64.get();
                format = 0;
            }
            bool halo_done = false;
            if (t->forward_engine) {
                // the last pass writes the halos itself (bins near both ends are stored twice): no copy launches
                const bool al = t->use_aligned();
                const FftEngine& eng = al ? *t->forward_aligned : *t->forward_engine;
                FftRowWindow w = al ? (t->windowed_aligned ? t->window_aligned : FftRowWindow{0, (int)(t->n / eng.row_length()) - 1, 0})
                                    : (t->windowed ? t->window : FftRowWindow{0, (int)(t->n / eng.row_length()) - 1, 0});
                w.halo = (int)t->halo;
                halo_done = t->halo > 0;
                // (aligned plan: x -> the spectrum storage as scratch -> forward_tmp -> the spectrum, no pass in place)
                eng.c2c(static_cast<const float2*>(x), t->spectrum(), t->forward_tmp.as<float2>(), 1, false, 1.0f,
                        as_stream(stream), &w, al ? t->X.as<float2>() : nullptr, format);
            } else {
                t->forward_work.reserve(t->forward->work_bytes());
                t->forward->exec(const_cast<void*>(x), t->spectrum(), t->forward_work.get(), as_stream(stream));
            }
            if (t->halo && !halo_done) {
                float2* X = t->spectrum();
                const size_t hb = sizeof(float2) * (size_t)t->halo;
                RC_HIP(hipMemcpyAsync(X - t->halo, X + t->n - t->halo, hb, hipMemcpyDeviceToDevice, as_stream(stream)));
                RC_HIP(hipMemcpyAsync(X + t->n, X, hb, hipMemcpyDeviceToDevice, as_stream(stream)));
            }
        }
        t->set_loaded(true, t->forward_engine && (t->use_aligned() ? t->windowed_aligned : t->windowed), t->shard_first,
                      t->shard_count);
        t->set_held(0, t->n);
        if (t->loaded_windowed) {   // the rows the last pass of the plan that ran has stored
            const bool al = t->use_aligned();
            const FftRowWindow& w = al ? t->window_aligned : t->window;
            const int64_t f0 = (al ? *t->forward_aligned : *t->forward_engine).row_length(), rows = t->n / f0;
            t->set_held((int64_t)w.lo * f0, (((int64_t)w.hi - w.lo + rows) % rows + 1) * f0);
        }
        t->iq_after_load(as_stream(stream));   // rcfm_tuner_set_iq_balance; off (the default): nothing
    });
}

int rcfm_tuner_load(rcfm_tuner_t t, const void* x, void* stream) { return tuner_load(t, 0, x, stream); }

int rcfm_tuner_load_raw(rcfm_tuner_t t, int format, const void* x, void* stream) {
    if (format == 0) format = -1;   // 0 is tuner_load's complex64, not a format of this entry point
    return tuner_load(t, format, x, stream);
}

int rcfm_tuner_load_route(rcfm_tuner_t t, int format, int* route) {
    return guarded([&] {
        RC_REQUIRE(iq_format_ok(format), RCFM_ERR_ARG, "unknown IQ format (RCFM_IQ_CS16, RCFM_IQ_CS8, RCFM_IQ_CU8)");
        RC_REQUIRE(t && route, RCFM_ERR_ARG, "NULL argument");
        *route = t->raw_fused() ? 1 : 0;
    });
}

int rcfm_tuner_shard(rcfm_tuner_t t, int first, int count) {
    return guarded([&] {
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL argument");
        t->shard(first, count);
    });
}

int rcfm_tuner_run(rcfm_tuner_t t, int first, int count, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(t && out, RCFM_ERR_ARG, "NULL argument");
        ArenaScope scope(t->arena);
        t->run(first, count, static_cast<float2*>(out), as_stream(stream));
    });
}

int rcfm_tuner_levels(rcfm_tuner_t t, int first, int count, void* power, void* stream) {
    return guarded([&] {
        RC_REQUIRE(t && power, RCFM_ERR_ARG, "NULL argument");
        ArenaScope scope(t->arena);
        t->levels(first, count, static_cast<float*>(power), as_stream(stream));
    });
}

int rcfm_tuner_carriers(rcfm_tuner_t t, int first, int count, float gate, void* peak_bin, void* peak_power, void* centroid,
                        void* spread, void* stream) {
    return guarded([&] {
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(peak_bin || peak_power || centroid || spread, RCFM_ERR_ARG, "all four outputs are NULL");
        RC_REQUIRE(std::isfinite(gate) && gate >= 0.f, RCFM_ERR_ARG, "the gate must be finite and >= 0");
        ArenaScope scope(t->arena);
        t->carriers(first, count, (double)gate * (double)t->n * (double)t->n, static_cast<int32_t*>(peak_bin),
                    static_cast<float*>(peak_power), static_cast<float*>(centroid), static_cast<float*>(spread),
                    as_stream(stream));
    });
}

int rcfm_tuner_retune(rcfm_tuner_t t, int first, int count, const int64_t* roll_host, void* stream) {
    return guarded([&] {
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL handle");
        RC_REQUIRE(count <= 0 || roll_host != nullptr, RCFM_ERR_ARG, "roll is NULL");
        t->retune(first, count, roll_host, as_stream(stream));
    });
}

int rcfm_tuner_power_spectrum(rcfm_tuner_t t, int64_t first_bin, int64_t nbins, int64_t cells, void* power, void* peak,
                              void* stream) {
    return guarded([&] {
        RC_REQUIRE(t && (power || peak), RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(nbins >= 1 && cells >= 1 && cells <= nbins, RCFM_ERR_ARG, "a span has at least one bin and 1 .. nbins cells");
        RC_REQUIRE(first_bin >= -(t->n / 2) && nbins <= t->n && first_bin <= t->n - t->n / 2 - nbins, RCFM_ERR_ARG,
                   "the span leaves the signed bins [-floor(n / 2), n - floor(n / 2))");
        ArenaScope scope(t->arena);
        t->power_spectrum(first_bin, nbins, cells, static_cast<float*>(power), static_cast<float*>(peak), as_stream(stream));
    });
}

int rcfm_squelch(const void* power, const void* threshold, int count, size_t floats_per_channel, void* audio, void* open,
                 void* stream) {
    return guarded([&] {
        RC_REQUIRE(power && threshold, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(count >= 0, RCFM_ERR_ARG, "negative channel count");
        StageTimer tm(ST_SQUELCH, as_stream(stream));
        launch_squelch(static_cast<const float*>(power), static_cast<const float*>(threshold), count, floats_per_channel,
                       static_cast<float*>(audio), static_cast<uint8_t*>(open), as_stream(stream));
    });
}

int rcfm_tuner_spectrum(rcfm_tuner_t t, void** X) {
    return guarded([&] {
        RC_REQUIRE(t && X, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(!t->ext_window, RCFM_ERR_STATE, "a window is attached: the whole spectrum is not on this device");
        *X = t->spectrum();
    });
}

int rcfm_tuner_spectrum_layout(rcfm_tuner_t t, int64_t* halo, int64_t* n) {
    return guarded([&] {
        RC_REQUIRE(t && halo && n, RCFM_ERR_ARG, "NULL argument");
        *halo = t->halo;
        *n = t->n;
    });
}

int rcfm_tuner_attach_spectrum(rcfm_tuner_t t, void* storage, int loaded_first, int loaded_count) {
    return guarded([&] {
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL argument");
        if (loaded_count > 0) require_channels(loaded_first, loaded_count, t->nch);
        ArenaScope scope(t->arena);
        t->ext = static_cast<float2*>(storage);
        t->ext_window = false;
        // the handle's own [halo | n | halo] buffer is not needed while the caller supplies the storage
        const size_t own_bytes = t->own_spectrum_bytes();
        if (storage != nullptr) t->X.reset(0);
        else if (t->X.bytes() < own_bytes) t->X.reset(own_bytes);
        // what the storage holds: the bins of channels [loaded_first, loaded_first + loaded_count), or nothing yet
        int64_t fb = 0, nb = t->n;
        if (loaded_count > 0) t->bin_window(loaded_first, loaded_count, &fb, &nb);
        t->set_loaded(loaded_count > 0, nb < t->n, loaded_first, std::max(loaded_count, 0));
        t->set_held(fb, nb);
    });
}

int rcfm_tuner_window_layout(rcfm_tuner_t t, int first, int count, int64_t* halo, int64_t* nbins) {
    return guarded([&] {
        RC_REQUIRE(t && halo && nbins, RCFM_ERR_ARG, "NULL argument");
        int64_t fb = 0, nb = 0;
        t->window_storage(first, count, &fb, &nb);
        *halo = t->halo;
        *nbins = nb;
    });
}

int rcfm_tuner_attach_window(rcfm_tuner_t t, void* storage, int first, int count) {
    return guarded([&] {
        RC_REQUIRE(t && storage, RCFM_ERR_ARG, "NULL argument");
        int64_t fb = 0, nb = 0;
        t->window_storage(first, count, &fb, &nb);
        t->X.reset(0);
        // bin b of the window sits at storage[halo + b - fb]: `ext` is where bin -halo would be
        t->ext = static_cast<float2*>(storage) - fb;
        t->ext_window = true;
        t->ext_first = first;
        t->ext_count = count;
        t->set_loaded(false, false, first, 0);
    });
}

int rcfm_tuner_set_option(rcfm_tuner_t t, int option, int value) {
    return guarded([&] {
        RC_REQUIRE(t, RCFM_ERR_ARG, "NULL handle");
        switch (option) {
            case RCFM_TUNER_OPT_NARROW_TILES:
                RC_REQUIRE(value >= 0 && value <= 2, RCFM_ERR_ARG, "narrow tiles: 0 never, 1 automatic, 2 always");
                t->opt_narrow = value;
                break;
            case RCFM_TUNER_OPT_ALIGNED_PLAN: t->opt_aligned = value != 0; break;
            default: RC_REQUIRE(false, RCFM_ERR_ARG, "unknown tuner option");
        }
    });
}

int rcfm_tuner_window(rcfm_tuner_t t, int first, int count, int64_t* first_bin, int64_t* nbins) {
    return guarded([&] {
        RC_REQUIRE(t && first_bin && nbins, RCFM_ERR_ARG, "NULL argument");
        require_channels(first, count, t->nch);
        t->bin_window(first, count, first_bin, nbins);
    });
}

int rcfm_tuner_adopt(rcfm_tuner_t t, int first, int count, void* stream) {
    return guarded([&] {
        RC_REQUIRE(t != nullptr, RCFM_ERR_ARG, "NULL argument");
        t->adopt(first, count, as_stream(stream));
    });
}

int rcfm_tuner_destroy(rcfm_tuner_t t) {
    return guarded([&] { delete t; });
}

}  // extern "C"
