// Host-side table of csrc/spectrum_rules.h for tests/test_spectrum_rules.py: reads one request per line from
// standard input and prints what the rules return, one line per bin.  No HIP runtime call, no device.
//   H n                        k  hilbert_weight(n, k, 1)
//   R n m                      k  (k <= m / 2) resample_nyquist(1, k, ...) real_bin_is_real(k, m)   [first line: bin factor]
//   F m                        k  fold(k, m).kk .mirrored
//   P n re0 im0 re1 im1 ...    k  pair_even / 2, pair_odd / 2 of U[k], U[-k]
//   U n m re0 im0 ...          k  (k < m) stereo_unpack_point of U (length n) with weight 1, kept band kk < min(n, m) / 2 + 1
//   G B nyq nneg mode          k  gather_offset general form: d ok, nyquist_up_halved, and the plain form
//   S m kmax nyq_bin factor lower   k  ssb_kept, ssb_weights(1, ...) of the folded bin
#include "spectrum_rules.h"

#include <cstdio>
#include <vector>

using namespace rcfm;

static std::vector<float2> read_bins(int n) {
    std::vector<float2> u(n);
    for (auto& v : u)
        if (scanf("%f %f", &v.x, &v.y) != 2) v = make_float2(0.f, 0.f);
    return u;
}

int main() {
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'H') {
            int n;
            if (scanf("%d", &n) != 1) return 1;
            for (int k = 0; k < n; ++k) printf("H %d %d %.9g\n", n, k, hilbert_weight(n, k, 1.f));
        } else if (op == 'R') {
            int n, m;
            if (scanf("%d %d", &n, &m) != 2) return 1;
            const int bin = resample_nyquist_bin(n, m);
            const float factor = resample_nyquist_factor(n, m);
            printf("R %d %d bin %d %.9g\n", n, m, bin, factor);
            for (int k = 0; k <= m / 2; ++k) {
                const float2 y = resample_nyquist(make_float2(1.f, 1.f), k, bin, factor);
                printf("R %d %d %d %.9g %.9g %d\n", n, m, k, resample_nyquist(1.f, k, bin, factor), y.y, (int)real_bin_is_real(k, m));
            }
        } else if (op == 'F') {
            int m;
            if (scanf("%d", &m) != 1) return 1;
            for (int k = 0; k < m; ++k) printf("F %d %d %d %d\n", m, k, fold(k, m).kk, (int)fold(k, m).mirrored);
        } else if (op == 'P') {
            int n;
            if (scanf("%d", &n) != 1) return 1;
            const std::vector<float2> u = read_bins(n);
            for (int k = 0; k < n; ++k) {
                const float2 a = u[k], b = u[k == 0 ? 0 : n - k];
                const float2 e = pair_even(a, b), o = pair_odd(a, b);
                printf("P %d %d %.9g %.9g %.9g %.9g\n", n, k, 0.5f * e.x, 0.5f * e.y, 0.5f * o.x, 0.5f * o.y);
            }
        } else if (op == 'U') {
            int n, m;
            if (scanf("%d %d", &n, &m) != 2) return 1;
            const std::vector<float2> u = read_bins(n);
            const int nyq = (n < m ? n : m) / 2 + 1;
            for (int k = 0; k < m; ++k) {
                const Folded<int> f = fold(k, m);
                const bool live = f.kk < nyq;
                const float2 a = u[live ? f.kk : 0], b = u[live && f.kk > 0 ? n - f.kk : 0];
                const float2 v = stereo_unpack_point(a, b, 1.f, f, live, resample_nyquist_bin(n, m), resample_nyquist_factor(n, m), m);
                printf("U %d %d %d %.9g %.9g\n", n, m, k, v.x, v.y);
            }
        } else if (op == 'G') {
            int B, nyq, nneg, mode;
            if (scanf("%d %d %d %d", &B, &nyq, &nneg, &mode) != 4) return 1;
            for (int k = 0; k < B; ++k) {
                bool ok;
                const int d = gather_offset(k, B, nyq, nneg, mode, ok);
                printf("G %d %d %d %d %d %d %d %d %d\n", B, nyq, nneg, mode, k, d, (int)ok, (int)nyquist_up_halved(k, B, nyq),
                       gather_offset(k, B, nyq));
            }
        } else if (op == 'S') {
            int m, kmax, bin, lower;
            float factor;
            if (scanf("%d %d %d %f %d", &m, &kmax, &bin, &factor, &lower) != 5) return 1;
            for (int k = 0; k < m; ++k) {
                const Folded<int> f = fold(k, m);
                const float2 w = ssb_weights(1.f, f.kk, kmax, f.mirrored, lower != 0, bin, factor);
                printf("S %d %d %d %d %d %d %.9g %.9g\n", m, kmax, bin, lower, k, (int)ssb_kept(f.kk, kmax), w.x, w.y);
            }
        } else {
            return 1;
        }
    }
    return 0;
}
