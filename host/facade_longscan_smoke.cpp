// host/facade_longscan_smoke.cpp -- maxiLongScanBank of include/maximilian_bank.hpp from plain C++ (no HIP headers): a recording
// filtered where it lies.  Noise is put into a maxiLooperBank slot, the slot is filtered IN PLACE by a one-voice low-pass biquad
// (mxg_scan_long_render, K28: 5 chunks, a K10 block of 256 and 44 plain steps), and downloaded: bit for bit the library's host twin
// over the same samples, and within the biquad's bound of the direct-form-II recurrence written out here.  Then three lags over a
// block [N][3], out of place, two carried calls: the twin's bits, within the lag's bound of mxg_lag_host, and the state handed to
// the sequential maxiLagExpBank.  Exit status 0 = all of it held.
//
//   facade_longscan_smoke
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            fprintf(stderr, "facade_longscan_smoke: %s failed\n", #c);     \
            fails++;                                                       \
        }                                                                  \
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
        unsigned long long seed = 28;
        auto noise = [&]() {
            seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
            return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0;
        };

        // 1. a looper slot through a one-voice biquad, in place
        const size_t n = 5 * 2048 + 300;
        std::vector<double> rec(n);
        for (double &s : rec) s = noise();
        maxiLooperBank looper(1, n);
        looper.setSample(0, rec);
        maxiLongScanBank lp(1, maxiLongScanBank::BIQUAD);
        lp.setBiquad({0}, {1200.0}, {0.7}, {0.0});
        lp.process(n, looper.deviceSamples(0), looper.deviceSamples(0));
        const std::vector<double> got = looper.download(0);

        std::vector<double> twin(n), st(3, 0.0), seq(n);
        lp.host(n, rec.data(), twin.data(), st);
        EXPECT(same(got, twin));
        EXPECT(same(lp.state(), st));
        const std::vector<double> &c = lp.coefficients();  // a0, a1, a2, b1, b2
        double v1 = 0.0, v2 = 0.0;
        for (size_t i = 0; i < n; i++) {  // maxiBiquad::play, H:1360-1367
            const double v0 = rec[i] - (c[3] * v1) - (c[4] * v2);
            seq[i] = (c[0] * v0) + (c[1] * v1) + (c[2] * v2);
            v2 = v1;
            v1 = v0;
        }
        const double e1 = scaled_err(got, seq, 1, 0);
        printf("facade_longscan_smoke: biquad over a looper slot, |long - sequential| / peak = %.3e\n", e1);
        EXPECT(e1 <= 4e-10);

        // 2. three lags, out of place, two carried calls, then on with the sequential bank
        const size_t V = 3, N = 3 * 2048 + 5 * 64 + 7;
        const std::vector<double> alpha = {0.01, 0.1, 0.5};
        std::vector<double> x(2 * N * V), recip(V), val(V, 0.25), exp(2 * N * V), twin2(2 * N * V), st2(V, 0.25);
        for (double &s : x) s = noise();
        for (size_t v = 0; v < V; v++) recip[v] = 1.0 - alpha[v];
        maxiLongScanBank lag(V, maxiLongScanBank::LAG);
        lag.setLag(alpha);
        lag.set_state(st2);
        DeviceArray<double> d_x(2 * N * V, false), d_y(2 * N * V, false);
        d_x.upload(x);
        for (size_t b = 0; b < 2; b++) {
            lag.process(N, d_x.get() + b * N * V, d_y.get() + b * N * V);
            lag.host(N, x.data() + b * N * V, twin2.data() + b * N * V, st2);
        }
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> y = d_y.download();
        EXPECT(same(y, twin2));
        EXPECT(same(lag.state(), st2));
        maxigpu::check(mxg_lag_host(V, 2 * N, x.data(), alpha.data(), recip.data(), 0, val.data(), exp.data()), "mxg_lag_host");
        for (size_t v = 0; v < V; v++) EXPECT(scaled_err(y, exp, V, v) <= 9e-12);

        // refused by name
        EXPECT(mxg_scan_long_render(0, 0, 64, d_x.get(), d_x.get(), d_x.get(), d_y.get(), nullptr) < 0 && strstr(mxg_last_error(), "V = 0"));
        EXPECT(mxg_scan_long_render(0, 1, 0, d_x.get(), d_x.get(), d_x.get(), d_y.get(), nullptr) < 0 && strstr(mxg_last_error(), "N = 0"));
        EXPECT(mxg_scan_long_render(6, 1, 64, d_x.get(), d_x.get(), d_x.get(), d_y.get(), nullptr) < 0 && strstr(mxg_last_error(), "kind 6"));
        EXPECT(mxg_scan_long_render(5, 1, 64, d_x.get(), d_x.get(), d_y.get(), d_x.get() + 1, nullptr) < 0 && strstr(mxg_last_error(), "overlaps"));
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_longscan_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_longscan_smoke: ok\n");
    return 0;
}
