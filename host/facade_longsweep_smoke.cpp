// host/facade_longsweep_smoke.cpp -- maxiLongScanBank::processSwept of include/maximilian_bank.hpp from plain C++ (no HIP headers):
// a stem filtered by a lores whose cutoff and resonance move every sample (mxg_scan_long_render_swept, K31: 5 chunks of 1024, a
// block of 256 and 44 plain steps; cutoff on a 2 Hz LFO 200 Hz ... 8 kHz, resonance on a 3 Hz LFO 1 ... 30), in place, the
// coefficients from sweepCoefficients ([N][3][V]): bit for bit the library's host twin, and within the bound of the sequential
// recurrence written out here.  Then three lags whose alpha moves, packed [N][2][V], out of place, two carried calls: the twin's
// bits, within the bound of mxg_lag_host with alpha_per_sample = 1.  Exit status 0 = all of it held.
//
//   facade_longsweep_smoke
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                           \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "facade_longsweep_smoke: %s failed\n", #c);     \
            fails++;                                                        \
        }                                                                   \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}

static double scaled_err(const std::vector<double> &got, const std::vector<double> &exp, size_t V, size_t v) {
    double peak = 1e-300, err = 0.0;
    for (size_t i = v; i < exp.size(); i += V) {
        peak = fmax(peak, fabs(exp[i]));
        err = fmax(err, fabs(got[i] - exp[i]));
    }
    return err / peak;
}

int main() {
    try {
        maxiSettings::setup(44100, 2, 512);
        unsigned long long seed = 31;
        auto noise = [&]() {
            seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
            return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
        };
        const double twopi = 6.283185307179586;

        // 1. one stem through a swept lores, in place
        const size_t n = 5 * 1024 + 300;
        std::vector<double> stem(n), cutoff(n), res(n);
        for (size_t i = 0; i < n; i++) {
            stem[i] = noise();
            cutoff[i] = 200.0 + 7800.0 * (0.5 + 0.5 * sin(twopi * 2.0 * (double)i / 44100.0));
            res[i] = 1.0 + 29.0 * (0.5 + 0.5 * sin(twopi * 3.0 * (double)i / 44100.0));
        }
        const std::vector<double> cps = maxiLongScanBank::sweepCoefficients(maxiLongScanBank::LORES, n, 1, cutoff, res);  // [n][3][1]
        maxiLongScanBank lp(1, maxiLongScanBank::LORES);
        std::vector<double> st0 = {0.25, -0.5, 7.0, 8.0, 9.0};  // (rows 2-4 are not the scan's)
        lp.set_state(st0);
        DeviceArray<double> d_stem(n, false), d_cps(3 * n, false);
        d_stem.upload(stem);
        d_cps.upload(cps);
        lp.processSwept(n, d_stem.get(), d_cps.get(), 3, d_stem.get());
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> got = d_stem.download();

        std::vector<double> twin(n), st = st0, seq(n);
        lp.hostSwept(n, stem.data(), cps.data(), 3, twin.data(), st);
        EXPECT(same(got, twin));
        EXPECT(same(lp.state(), st));
        EXPECT(st[2] == 7.0 && st[3] == 8.0 && st[4] == 9.0);
        double x = st0[0], y = st0[1];
        for (size_t i = 0; i < n; i++) {  // maxiFilter::lores, C:455-468, c and r of sample i
            x = x + (stem[i] - y) * cps[3 * i];
            y = y + x;
            x = x * cps[3 * i + 1];
            seq[i] = y;
        }
        const double e1 = scaled_err(got, seq, 1, 0);
        printf("facade_longsweep_smoke: swept lores over a stem, |long - sequential| / peak = %.3e\n", e1);
        EXPECT(e1 <= 6e-12);

        // 2. three lags with moving alpha, out of place, two carried calls
        const size_t V = 3, N = 3 * 1024 + 5 * 64 + 7;
        std::vector<double> in(2 * N * V), aps(2 * N * V), rps(2 * N * V), c2(2 * N * 2 * V), val(V, 0.25), exp(2 * N * V), twin2(2 * N * V), st2(V, 0.25);
        for (double &s : in) s = noise();
        for (size_t i = 0; i < 2 * N; i++)
            for (size_t v = 0; v < V; v++) {
                const double a = 1e-4 + 0.9 * (0.5 + 0.5 * sin(twopi * (1.0 + (double)v) * (double)i / 44100.0));
                aps[i * V + v] = c2[(i * 2) * V + v] = a;
                rps[i * V + v] = c2[(i * 2 + 1) * V + v] = 1.0 - a;
            }
        maxiLongScanBank lag(V, maxiLongScanBank::LAG);
        lag.set_state(st2);
        DeviceArray<double> d_x(2 * N * V, false), d_c(2 * N * 2 * V, false), d_y(2 * N * V, false);
        d_x.upload(in);
        d_c.upload(c2);
        for (size_t b = 0; b < 2; b++) {
            lag.processSwept(N, d_x.get() + b * N * V, d_c.get() + b * N * 2 * V, 2, d_y.get() + b * N * V);
            lag.hostSwept(N, in.data() + b * N * V, c2.data() + b * N * 2 * V, 2, twin2.data() + b * N * V, st2);
        }
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> yv = d_y.download();
        EXPECT(same(yv, twin2));
        EXPECT(same(lag.state(), st2));
        maxigpu::check(mxg_lag_host(V, 2 * N, in.data(), aps.data(), rps.data(), 1, val.data(), exp.data()), "mxg_lag_host");
        for (size_t v = 0; v < V; v++) EXPECT(scaled_err(yv, exp, V, v) <= 5e-12);

        // refused by name
        EXPECT(mxg_scan_long_render_swept(2, 1, 64, d_x.get(), d_c.get(), 2, d_y.get(), d_y.get(), nullptr) < 0 && strstr(mxg_last_error(), "no swept form"));
        EXPECT(mxg_scan_long_render_swept(3, 1, 64, d_x.get(), d_c.get(), 1, d_y.get(), d_y.get(), nullptr) < 0 && strstr(mxg_last_error(), "coef_rows = 1"));
        EXPECT(mxg_scan_long_render_swept(5, 1, 64, d_x.get(), d_c.get(), 2, d_y.get(), d_c.get() + 8, nullptr) < 0 && strstr(mxg_last_error(), "coef_ps"));
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_longsweep_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_longsweep_smoke: ok\n");
    return 0;
}
