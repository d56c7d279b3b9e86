// Single-stage entry points outside the handles' chains: the resampler, FIR filters, the analytic signal, the PLL
// phase, the discriminator and the FFT engine / rocFFT transforms (rcfm_fft_*).

#include <cmath>
#include <cstring>
#include <tuple>

#include "agc.h"
#include "api_internal.h"

using namespace rcfm;

struct rcfm_resampler_s {
    int C = 0;
    int64_t n = 0, m = 0;
    bool cplx = false;
    ResampleGeom geom;
    std::unique_ptr<FftPlan> fwd, inv;
    DeviceBuffer spec_in, spec_out, work;
    // complex down-sampling on the FFT engine: forward transform, then the Tuner's fused gather + window +
    // inverse transform with roll = 0 and the Hamming weight (the same math, decimate.py:47-48 vs tuner.py:159-161)
    std::unique_ptr<FftEngine> eng_n, eng_m;
    DeviceBuffer tmp_n, tmp_m, zero_roll;
    // only bins |k| <= m/2 of the long spectrum are read: its last pass stores just the rows that hold them
    bool windowed = false;
    FftRowWindow window{0, 0};
};

namespace {

// Device copies of filter taps, keyed by their values: Bandpass / Deemphasis hand the same host array to every call
// (bandpass.py:72, deemphasis.py:64), so after the first call nothing is allocated, uploaded or waited for.
// The caller holds a shared_ptr across its launch: an eviction on another thread cannot free taps a kernel is about
// to be launched with (the buffer dies when the last holder lets go; hipFree then orders itself behind the launch).
// At most 64 sets are kept, least recently used out first, one per miss.
std::shared_ptr<DeviceBuffer> cached_taps(const std::vector<float>& taps) {
    struct Entry {
        std::shared_ptr<DeviceBuffer> buf;
        uint64_t used;
    };
    static std::mutex mu;
    static std::map<std::vector<float>, Entry> cache;
    static uint64_t tick = 0;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(taps);
    if (it == cache.end()) {
        if (cache.size() >= 64) {
            auto oldest = cache.begin();
            for (auto e = cache.begin(); e != cache.end(); ++e)
                if (e->second.used < oldest->second.used) oldest = e;
            cache.erase(oldest);
        }
        auto buf = std::make_shared<DeviceBuffer>();
        buf->upload(taps.data(), taps.size() * sizeof(float));
        it = cache.emplace(taps, Entry{std::move(buf), 0}).first;
    }
    it->second.used = ++tick;
    return it->second.buf;
}

// Plans and workspaces of rcfm_hilbert: PLL.step (pll.py:25-34) is called once per buffer with the same geometry,
// so nothing is planned, allocated or synchronised after the first call.  The key includes the device and the
// STREAM: calls on one stream are ordered by that stream and may share spec / tmp; two PLLs on different streams
// (or threads) get separate workspaces instead of racing on one.  At most 16 entries are kept, least recently
// used out first (hipFree waits for the device, so an evicted workspace is never freed under a running kernel).
struct HilbertPlan {
    std::unique_ptr<FftEngine> eng;            // engine lengths: real -> full spectrum -> masked inverse transform
    std::unique_ptr<FftPlan> fwd, inv;         // otherwise rocFFT (r2c, mask kernel, c2c inverse)
    DeviceBuffer spec, tmp, work;
    uint64_t used = 0;
};
using HilbertKey = std::tuple<int, hipStream_t, int, int>;   // device, stream, n, C
HilbertPlan& hilbert_plan(int n, int C, hipStream_t s) {
    static std::map<HilbertKey, std::unique_ptr<HilbertPlan>> plans;
    static uint64_t tick = 0;
    int dev = 0;
    RC_HIP(hipGetDevice(&dev));
    const HilbertKey key{dev, s, n, C};
    auto it = plans.find(key);
    if (it == plans.end()) {
        if (plans.size() >= 16) {
            auto oldest = plans.begin();
            for (auto e = plans.begin(); e != plans.end(); ++e)
                if (e->second->used < oldest->second->used) oldest = e;
            plans.erase(oldest);
        }
        auto p = std::make_unique<HilbertPlan>();
        FftPlanDesc probe;
        if (use_engine() && fft_plan_describe(n, &probe)) {
            p->eng = std::make_unique<FftEngine>(n);
            p->spec.reset((size_t)C * n * sizeof(float2));
            p->tmp.reset((size_t)C * p->eng->tmp_stride() * sizeof(float2));
        } else {
            p->fwd = std::make_unique<FftPlan>(FftKind::R2C, (size_t)n, (size_t)C, false);
            p->inv = std::make_unique<FftPlan>(FftKind::C2C_INVERSE, (size_t)n, (size_t)C, true);
            p->spec.reset((size_t)C * (n / 2 + 1) * sizeof(float2));
            p->work.reserve(std::max(p->fwd->work_bytes(), p->inv->work_bytes()));
        }
        it = plans.emplace(key, std::move(p)).first;
    }
    it->second->used = ++tick;
    return *it->second;
}
std::mutex g_hilbert_mu;

// every batched entry point carries the signal index in a grid y / z coordinate (kernels.h)
const char* const kBatchLimit = "at most 65535 signals per call";
static_assert(kMaxBatch == 65535, "kBatchLimit and rcfm.h state the batch limit in words");
}  // namespace

extern "C" {

// ---- primitives --------------------------------------------------------------

int rcfm_resampler_create(int C, int n, int m, int is_complex, rcfm_resampler_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "out is NULL");
        RC_REQUIRE(C >= 1 && n >= 1 && m >= 1, RCFM_ERR_ARG, "bad resampler size");
        RC_REQUIRE(C <= kMaxBatch, RCFM_ERR_ARG, kBatchLimit);
        auto r = std::make_unique<rcfm_resampler_s>();
        r->C = C;
        r->n = n;
        r->m = m;
        r->cplx = is_complex != 0;
        r->geom.build(n, m, 0.54, r->cplx);
        FftPlanDesc probe;
        if (r->cplx && use_engine() && m <= n && fft_plan_describe(n, &probe) && fft_plan_describe(m, &probe)) {
            r->eng_n = std::make_unique<FftEngine>(n);
            r->eng_m = std::make_unique<FftEngine>(m);
            r->spec_in.reset((size_t)C * n * sizeof(float2));
            r->tmp_n.reset((size_t)C * r->eng_n->tmp_stride() * sizeof(float2));
            r->tmp_m.reset((size_t)C * r->eng_m->tmp_stride() * sizeof(float2));
            std::vector<int64_t> zeros((size_t)C, 0);
            r->zero_roll.upload(zeros.data(), zeros.size() * sizeof(int64_t));
            const int64_t n1 = r->eng_n->row_length(), rows = n / n1;
            const int64_t hi = (r->geom.nyq + 1) / n1;                        // last row of the positive bins
            const int64_t lo = (n - r->geom.nneg - 2) / n1;                   // first row of the negative bins
            if (C == 1 && lo > hi + 1 && lo < rows) {                         // (rows are counted per signal)
                r->windowed = true;
                r->window = FftRowWindow{(int)lo, (int)hi};
            }
            *out = r.release();
            return;
        }
        if (r->cplx) {
            r->fwd = std::make_unique<FftPlan>(FftKind::C2C_FORWARD, (size_t)n, (size_t)C, false);
            r->inv = std::make_unique<FftPlan>(FftKind::C2C_INVERSE, (size_t)m, (size_t)C, true);
            r->spec_in.reset((size_t)C * n * sizeof(float2));
        } else {
            r->fwd = std::make_unique<FftPlan>(FftKind::R2C, (size_t)n, (size_t)C, false);
            r->inv = std::make_unique<FftPlan>(FftKind::C2R, (size_t)m, (size_t)C, false);
            r->spec_in.reset((size_t)C * (n / 2 + 1) * sizeof(float2));
            r->spec_out.reset((size_t)C * (m / 2 + 1) * sizeof(float2));
        }
        r->work.reserve(std::max(r->fwd->work_bytes(), r->inv->work_bytes()));
        *out = r.release();
    });
}

int rcfm_resampler_run(rcfm_resampler_t r, const void* in, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(r && in && out, RCFM_ERR_ARG, "NULL argument");
        hipStream_t s = as_stream(stream);
        const ResampleGeom& g = r->geom;
        if (r->eng_n) {
            r->eng_n->c2c(static_cast<const float2*>(in), r->spec_in.as<float2>(), r->tmp_n.as<float2>(), r->C, false,
                          1.0f, s, r->windowed ? &r->window : nullptr);
            TunerGather tg{r->spec_in.as<float2>(), r->n, r->zero_roll.as<int64_t>(), 0.54, g.nyq, g.nneg, g.nyq_mode,
                           nullptr, 0, r->n};
            fused_tuner_ifft(*r->eng_m, tg, static_cast<float2*>(out), r->tmp_m.as<float2>(), r->C, s);
            return;
        }
        if (r->cplx) {
            r->fwd->exec(const_cast<void*>(in), r->spec_in.get(), r->work.get(), s);
            launch_spectrum_c2c(r->spec_in.as<float2>(), r->n, r->n, nullptr, static_cast<float2*>(out), r->m,
                                r->C, g.wpos.as<float>(), g.wneg.as<float>(), g.w_merge, g.nyq, g.nneg,
                                g.nyq_mode, g.scale, s);
            r->inv->exec(out, out, r->work.get(), s);
        } else {
            r->fwd->exec(const_cast<void*>(in), r->spec_in.get(), r->work.get(), s);
            launch_spectrum_r2c(r->spec_in.as<float2>(), r->n, r->spec_out.as<float2>(), r->m, r->C,
                                g.wr.as<float>(), g.nyq, g.nyq_bin, g.nyq_factor, g.scale, s);
            r->inv->exec(r->spec_out.get(), out, r->work.get(), s);
        }
    });
}

int rcfm_resampler_destroy(rcfm_resampler_t r) {
    return guarded([&] { delete r; });
}

int rcfm_filtfilt(int C, int n, const float* taps_host, int ntaps, const void* x, void* y, void* stream) {
    return guarded([&] {
        RC_REQUIRE(taps_host && x && y, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1 && ntaps >= 1, RCFM_ERR_ARG, "bad filtfilt size");
        RC_REQUIRE(C <= kMaxBatch, RCFM_ERR_ARG, kBatchLimit);
        RC_REQUIRE(ntaps <= kPilotMaxTaps, RCFM_ERR_ARG,
                   "rcfm_filtfilt takes at most " + std::to_string(kPilotMaxTaps) + " taps");
        RC_REQUIRE(n > 3 * ntaps, RCFM_ERR_ARG,
                   "The length of the input vector x must be greater than padlen, which is " +
                       std::to_string(3 * ntaps) + ".");
        hipStream_t s = as_stream(stream);
        const std::shared_ptr<DeviceBuffer> gd = cached_taps(zero_phase_kernel(taps_host, ntaps));
        launch_pilot_stage(nullptr, static_cast<const float*>(x), nullptr, static_cast<float*>(y), n, C,
                           gd->as<float>(), ntaps - 1, 0.f, s);
    });
}

int rcfm_lfilter_fir(int C, int n, const float* taps_host, int ntaps, void* state, const void* x, void* y,
                     void* stream) {
    return guarded([&] {
        RC_REQUIRE(taps_host && x && y && (state || ntaps < 2), RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1 && n >= 1 && ntaps >= 1, RCFM_ERR_ARG, "bad lfilter size");
        RC_REQUIRE(C <= kMaxBatch, RCFM_ERR_ARG, kBatchLimit);
        RC_REQUIRE(ntaps <= kFirMaxTaps, RCFM_ERR_ARG,
                   "rcfm_lfilter_fir takes at most " + std::to_string(kFirMaxTaps) + " taps");
        // k_fir's workgroups read the previous tile's tail of x while others write y, and k_fir_state reads x after y is
        // complete: in place, both would see outputs where they need inputs
        {
            const char* xb = static_cast<const char*>(x);
            const char* yb = static_cast<const char*>(y);
            const size_t bytes = (size_t)C * (size_t)n * sizeof(float);
            RC_REQUIRE(xb + bytes <= yb || yb + bytes <= xb, RCFM_ERR_ARG,
                       "rcfm_lfilter_fir does not run in place: x and y must not overlap");
        }
        hipStream_t s = as_stream(stream);
        const std::shared_ptr<DeviceBuffer> td = cached_taps(std::vector<float>(taps_host, taps_host + ntaps));
        launch_fir(static_cast<const float*>(x), static_cast<float*>(y), n, 1, C, td->as<float>(), ntaps,
                   static_cast<const float*>(state), nullptr, s);
        launch_fir_state(static_cast<const float*>(x), n, 1, C, td->as<float>(), ntaps, static_cast<float*>(state), s);
    });
}

int rcfm_agc(int C, int n, int mode, double decay_samples, float level, float floor, void* state, const void* v,
             void* audio, void* stream) {
    return guarded([&] {
        RC_REQUIRE(state && v && audio, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1 && n >= 1, RCFM_ERR_ARG, "bad agc size");
        RC_REQUIRE(C <= kMaxBatch, RCFM_ERR_ARG, kBatchLimit);
        RC_REQUIRE(mode == RCFM_AGC_PEAK || mode == RCFM_AGC_CARRIER, RCFM_ERR_ARG, "unknown AGC mode");
        RC_REQUIRE(std::isfinite(decay_samples) && decay_samples > 0.0, RCFM_ERR_ARG, "AGC decay_samples must be finite and > 0");
        RC_REQUIRE(std::isfinite(level) && level > 0.f, RCFM_ERR_ARG, "AGC level must be finite and > 0");
        RC_REQUIRE(std::isfinite(floor) && floor >= 0.f, RCFM_ERR_ARG, "AGC floor must be finite and >= 0");
        {   // a row is staged whole before it is stored, so in place works; a shifted overlap would read rows already written
            const char* xb = static_cast<const char*>(v);
            const char* yb = static_cast<const char*>(audio);
            const size_t bytes = (size_t)C * (size_t)n * sizeof(float);
            RC_REQUIRE(xb == yb || xb + bytes <= yb || yb + bytes <= xb, RCFM_ERR_ARG,
                       "rcfm_agc runs in place (audio == v) or on separate arrays: partial overlap");
        }
        launch_agc_tail(mode, static_cast<const float*>(v), static_cast<float*>(audio), n, C,
                        agc_params(decay_samples, level, floor), static_cast<float*>(state), as_stream(stream));
    });
}

int rcfm_hilbert(int C, int n, const void* x, void* z, void* stream) {
    return guarded([&] {
        RC_REQUIRE(x && z, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1 && n >= 1, RCFM_ERR_ARG, "bad hilbert size");
        RC_REQUIRE(C <= kMaxBatch, RCFM_ERR_ARG, kBatchLimit);
        hipStream_t s = as_stream(stream);
        std::lock_guard<std::mutex> lock(g_hilbert_mu);   // the cache itself; the kernels are ordered by their stream
        HilbertPlan& p = hilbert_plan(n, C, s);
        if (p.eng) {
            fused_real_fft(*p.eng, static_cast<const float*>(x), p.spec.as<float2>(), p.tmp.as<float2>(), C,
                           kKeepLowerHalf /* bins above n/2 are never read */, s);
            fused_hilbert_ifft(*p.eng, p.spec.as<float2>(), static_cast<float2*>(z), p.tmp.as<float2>(), C, s);
            return;
        }
        p.fwd->exec(const_cast<void*>(x), p.spec.get(), p.work.get(), s);
        launch_hilbert_mask(p.spec.as<float2>(), static_cast<float2*>(z), n, C, 1.0f / (float)n, s);
        p.inv->exec(z, z, p.work.get(), s);
    });
}

int rcfm_pll_phase(const void* z, size_t count, double mult, int want_imag, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(z && out, RCFM_ERR_ARG, "NULL argument");
        // one thread per sample, and a grid holds fewer than 2^32 threads
        RC_REQUIRE(count <= (size_t)4294967040u, RCFM_ERR_ARG, "at most 4294967040 samples per call");
        launch_pll_phase(static_cast<const float2*>(z), count, mult, want_imag, static_cast<float*>(out),
                         as_stream(stream));
    });
}

int rcfm_discriminator(int C, int n, const void* iq, void* d, void* stream) {
    return guarded([&] {
        RC_REQUIRE(iq && d, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(C >= 1 && n >= 1, RCFM_ERR_ARG, "bad discriminator size");
        RC_REQUIRE(C <= kMaxBatch, RCFM_ERR_ARG, kBatchLimit);
        launch_discriminator(static_cast<const float2*>(iq), static_cast<float*>(d), n, C, as_stream(stream));
    });
}

// ---- FFT engine --------------------------------------------------------------------

static_assert(sizeof(rcfm_fft_pass) == sizeof(FftPass), "ABI mirror of FftPass out of date");
static_assert(sizeof(rcfm_fft_plan) == sizeof(FftPlanDesc), "ABI mirror of FftPlanDesc out of date");

int rcfm_fft_describe(int64_t n, int max_l, rcfm_fft_plan* plan) {
    return guarded([&] {
        RC_REQUIRE(plan != nullptr, RCFM_ERR_ARG, "plan is NULL");
        FftPlanDesc d;
        RC_REQUIRE(fft_plan_describe(n, &d, max_l), RCFM_ERR_ARG, "length not supported by the FFT engine");
        std::memcpy(plan, &d, sizeof(d));
    });
}

int rcfm_fft_describe_plan(int64_t n, const int64_t* pass_lengths, int npass, int layout, rcfm_fft_plan* plan) {
    return guarded([&] {
        RC_REQUIRE(plan != nullptr && pass_lengths != nullptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(layout >= -1 && layout <= 2, RCFM_ERR_ARG, "layout: -1 automatic, 0 plain, 1 tile-blocked, 2 padded rows");
        FftPlanDesc d;
        RC_REQUIRE(fft_plan_describe(n, &d, 0, pass_lengths, npass, layout), RCFM_ERR_ARG,
                   "pass lengths not supported by the FFT engine");
        std::memcpy(plan, &d, sizeof(d));
    });
}

int rcfm_fft_c2c(int64_t n, int batch, int inverse, const void* in, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(in && out && batch >= 1, RCFM_ERR_ARG, "bad argument");
        static std::mutex mu;
        static std::map<int64_t, std::unique_ptr<FftEngine>> engines;
        static DeviceBuffer tmp;
        std::lock_guard<std::mutex> lock(mu);
        auto it = engines.find(n);
        if (it == engines.end()) it = engines.emplace(n, std::make_unique<FftEngine>(n)).first;
        tmp.reserve((size_t)batch * it->second->tmp_stride() * sizeof(float2));
        it->second->c2c(static_cast<const float2*>(in), static_cast<float2*>(out), tmp.as<float2>(), batch,
                        inverse != 0, 1.0f, as_stream(stream));
    });
}

int rcfm_fft_c2c_plan(int64_t n, const int64_t* pass_lengths, int npass, int layout, int batch, int inverse, const void* in,
                      void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(in && out && batch >= 1 && pass_lengths && npass >= 1 && npass <= kFftMaxPasses, RCFM_ERR_ARG, "bad argument");
        RC_REQUIRE(layout >= -1 && layout <= 2, RCFM_ERR_ARG, "layout: -1 automatic, 0 plain, 1 tile-blocked, 2 padded rows");
        static std::mutex mu;
        static std::map<std::vector<int64_t>, std::unique_ptr<FftEngine>> engines;
        static DeviceBuffer tmp, tmp2;
        std::lock_guard<std::mutex> lock(mu);
        std::vector<int64_t> key(pass_lengths, pass_lengths + npass);
        key.push_back(layout);
        auto it = engines.find(key);
        if (it == engines.end()) it = engines.emplace(key, std::make_unique<FftEngine>(n, pass_lengths, npass, layout)).first;
        const FftEngine& e = *it->second;
        RC_REQUIRE(e.desc().n == n, RCFM_ERR_ARG, "the pass lengths do not multiply to n");
        tmp.reserve((size_t)batch * e.tmp_stride() * sizeof(float2));
        // the padded-rows layout's intermediates do not fit `out`: a second scratch array, so that (like the default plan
        // of a transform beyond the Infinity Cache) no pass runs in place
        const bool second = layout == 2 && (size_t)n * (size_t)batch * sizeof(float2) > ((size_t)256 << 20);
        if (second) tmp2.reserve((size_t)batch * e.tmp_stride() * sizeof(float2));
        e.c2c(static_cast<const float2*>(in), static_cast<float2*>(out), tmp.as<float2>(), batch, inverse != 0, 1.0f,
              as_stream(stream), nullptr, second ? tmp2.as<float2>() : nullptr);
    });
}

int rcfm_fft_c2c_rocfft(int64_t n, int batch, int inverse, const void* in, void* out, void* stream) {
    return guarded([&] {
        RC_REQUIRE(in && out && batch >= 1 && n >= 1, RCFM_ERR_ARG, "bad argument");
        static std::mutex mu;
        static std::map<std::tuple<int64_t, int, int, int>, std::unique_ptr<FftPlan>> plans;
        static DeviceBuffer work;
        std::lock_guard<std::mutex> lock(mu);
        const bool in_place = (in == out);
        auto key = std::make_tuple(n, batch, inverse ? 1 : 0, in_place ? 1 : 0);
        auto it = plans.find(key);
        if (it == plans.end())
            it = plans.emplace(key, std::make_unique<FftPlan>(inverse ? FftKind::C2C_INVERSE : FftKind::C2C_FORWARD,
                                                               (size_t)n, (size_t)batch, in_place)).first;
        work.reserve(it->second->work_bytes());
        it->second->exec(const_cast<void*>(in), out, work.get(), as_stream(stream));
    });
}

}  // extern "C"
