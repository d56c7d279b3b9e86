// Host-side filter and window design: the scipy.signal equivalents the handles upload as device tables.

#include <cmath>

#include "api_internal.h"

namespace rcfm {

namespace {
// fftshift(get_window(name, n))[k]  (tuner.py:156-157, decimate.py:32-33): the periodic
// general-cosine window a0 - (1 - a0) cos(2 pi i / n) read at i = (k - n//2) mod n.
double shifted_window(double a0, int64_t n, int64_t k) {
    if (n == 1) return 1.0;
    int64_t i = (k - n / 2) % n;
    if (i < 0) i += n;
    return a0 - (1.0 - a0) * std::cos(2.0 * kPi * (double)i / (double)n);
}
}  // namespace

void ResampleGeom::build(int64_t n_, int64_t m_, double a0, bool complex_input) {
    n = n_;
    m = m_;
    const int nmin = (int)std::min(n, m);
    nyq = nmin / 2 + 1;
    scale = (float)(1.0 / (double)n);
    const bool even = (nmin % 2) == 0;
    if (complex_input) {
        nneg = nmin > 2 ? nmin - nyq : 0;
        std::vector<float> p(nyq), q(nneg + 1, 0.f);
        for (int k = 0; k < nyq; ++k) p[k] = (float)shifted_window(a0, n, k);
        for (int j = 1; j <= nneg; ++j) q[j] = (float)shifted_window(a0, n, n - j);
        wpos.upload(p.data(), p.size() * sizeof(float));
        wneg.upload(q.data(), q.size() * sizeof(float));
        nyq_mode = NYQ_NONE;
        if (even && m < n && nmin > 2) {   // (for nmin == 2 scipy's slice is empty)
            nyq_mode = NYQ_DOWN;
            w_merge = (float)shifted_window(a0, n, n - nmin / 2);
        } else if (even && n < m) {
            nyq_mode = NYQ_UP;
        }
    } else {
        // "Fold the window back on itself to mimic complex behavior"
        std::vector<float> r(nyq);
        for (int k = 0; k < nyq; ++k) {
            double w = shifted_window(a0, n, k);
            if (k >= 1) w = 0.5 * (w + shifted_window(a0, n, n - k));
            r[k] = (float)w;
        }
        wr.upload(r.data(), r.size() * sizeof(float));
        nyq_bin = resample_nyquist_bin(n, m);
        nyq_factor = resample_nyquist_factor(n, m);
    }
}

// firwin(numtaps, [lo, hi], pass_zero=False, window="hamm"), bandpass.py:50-52.
std::vector<double> firwin_bandpass(int numtaps, double lo, double hi) {
    std::vector<double> h(numtaps);
    const double alpha = 0.5 * (numtaps - 1);
    auto sinc = [](double x) { return x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x); };
    const double fc = 0.5 * (lo + hi);
    double s = 0.0;
    for (int i = 0; i < numtaps; ++i) {
        const double mm = i - alpha;
        const double win = numtaps == 1 ? 1.0 : 0.54 - 0.46 * std::cos(2.0 * kPi * i / (numtaps - 1));
        h[i] = (hi * sinc(hi * mm) - lo * sinc(lo * mm)) * win;
        s += h[i] * std::cos(kPi * mm * fc);
    }
    for (auto& v : h) v /= s;
    return h;
}

// g = b (*) reverse(b): the zero-phase kernel of filtfilt for an FIR b; returns g[centre..edge].
std::vector<float> zero_phase_kernel(const float* b, int nb) {
    std::vector<float> g(nb);
    for (int lag = 0; lag < nb; ++lag) {
        double acc = 0.0;
        for (int i = 0; i + lag < nb; ++i) acc += (double)b[i] * (double)b[i + lag];
        g[lag] = (float)acc;
    }
    return g;
}

// deemphasis.py:37-49: first 51 impulse-response samples of (1-x)/(z-x), then lfilter_zi.
void deemphasis_design(int64_t fs, double tau, float* taps51, float* zi50) {
    const double x = std::exp(-1.0 / ((double)fs * tau));
    double st = 0.0, u = 1.0;
    for (int i = 0; i < 51; ++i) {
        taps51[i] = (float)((1.0 - x) * st);
        st = x * st + u;
        u = 0.0;
    }
    // lfilter_zi for an FIR: zi[k] = sum_{j>k} b[j]  (float32 cumulative sum from the tail)
    float acc = 0.f;
    for (int k = 49; k >= 0; --k) {
        acc += taps51[k + 1];
        zi50[k] = acc;
    }
}

}  // namespace rcfm
