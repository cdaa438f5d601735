// host/facade_analysis_smoke.cpp -- maxiAnalysisBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference: the crossings are (prev <= 0 && x > 0) worked out here; the rate over a window of W samples is
// the number of crossings among the last W - 1 samples (what push, count += bit, count -= tail(W) leaves), for windows on both
// sides of a word of the ring and for W = capacity; the follower and the sample-and-hold are the same recurrences written out
// on the host; a stream rendered in uneven blocks equals the same stream rendered in one, state included; an output that is not
// asked for leaves its stage's state alone; the crossings drive maxiEnvGenBank as a trigger block on the device; a window of 0
// is refused and one above the capacity is held there and counted.  Exit status 0 = all of it held.
//
//   facade_analysis_smoke
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
            fprintf(stderr, "facade_analysis_smoke: %s failed\n", #c);     \
            fails++;                                                       \
        }                                                                  \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}

template <typename T>
static std::vector<T> fetch(const T *d, size_t n) {
    std::vector<T> h(n);
    maxigpu::check(mxg_sync(), "mxg_sync");
    maxigpu::check(mxg_memcpy_d2h(h.data(), d, n * sizeof(T), nullptr), "d2h");
    return h;
}

int main() {
    try {
        maxiSettings::setup(1000, 2, 512);
        const size_t V = 5, N = 777, cap = 130;
        const std::vector<uint32_t> window = {130, 129, 64, 37, 1};
        const std::vector<double> hold = {0.0, 1.0, 2.5, 37.0, 300.0};
        std::vector<double> x(N * V);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) {
                const double ph = fmod((double)n * (0.013 + 0.011 * (double)v) * (1.0 + (double)n / 900.0), 1.0);
                x[n * V + v] = (n % 97 < 5) ? 0.0 : (2.0 * ph - 1.0) * (0.25 + 0.75 * (double)((n / 50) % 3) / 2.0);
            }
        DeviceArray<double> dx(N * V), zx1(N * V), zc1(N * V), en1(N * V), sh1(N * V), zx2(N * V), zc2(N * V), en2(N * V), sh2(N * V);
        dx.upload(x);
        maxiAnalysisBank a(V, cap), b(V, cap);
        for (maxiAnalysisBank *k : {&a, &b}) {
            k->setWindow(window);
            k->setAttack(5);
            k->setRelease(50);
            k->setHold(hold);
        }
        a.render(N, dx.get(), zx1.get(), zc1.get(), en1.get(), sh1.get());
        const size_t cuts[] = {0, 1, 8, 9, 64, 130, 131, 300, 513, N};
        for (size_t k = 0; k + 1 < sizeof(cuts) / sizeof(cuts[0]); k++) {
            const size_t n0 = cuts[k], n = cuts[k + 1] - cuts[k];
            b.render(n, dx.get() + n0 * V, zx2.get() + n0 * V, zc2.get() + n0 * V, en2.get() + n0 * V, sh2.get() + n0 * V);
        }
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> hz = zx1.download(), hc = zc1.download(), he = en1.download(), hs = sh1.download();
        EXPECT(same(hz, zx2.download()) && same(hc, zc2.download()) && same(he, en2.download()) && same(hs, sh2.download()));
        EXPECT(fetch(a.ring(), 3 * V) == fetch(b.ring(), 3 * V) && fetch(a.ringPosition(), V) == fetch(b.ringPosition(), V));
        EXPECT(fetch(a.runningCount(), V) == fetch(b.runningCount(), V) && same(fetch(a.envelope(), V), fetch(b.envelope(), V)));
        EXPECT(same(fetch(a.holdPhase(), V), fetch(b.holdPhase(), V)) && same(fetch(a.holdValue(), V), fetch(b.holdValue(), V)));
        // by hand
        const double att = mxg_envfollow_coeff_host(5, 1000.0), rel = mxg_envfollow_coeff_host(50, 1000.0);
        EXPECT(att == pow(0.01, 1.0 / (5.0 * 1000.0 * 0.001)) && att > 0 && att < rel && rel < 1);
        size_t crossings = 0;
        bool ok_zx = true, ok_zc = true, ok_en = true, ok_sh = true;
        for (size_t v = 0; v < V; v++) {
            double prev = 0.0, env = 0.0, phase = 0.0, value = 0.0;
            const double hs_samples = (double)(size_t)(hold[v] / 1000.0 * 1000.0);
            for (size_t n = 0; n < N; n++) {
                const double s = x[n * V + v];
                const double bit = (prev <= 0 && s > 0) ? 1.0 : 0.0;
                prev = s;
                crossings += (size_t)bit;
                ok_zx = ok_zx && hz[n * V + v] == bit;
                double cnt = 0;  // the crossings among the last W - 1 samples
                for (size_t k = 0; k + 1 < window[v] && k <= n; k++) cnt += hz[(n - k) * V + v];
                ok_zc = ok_zc && hc[n * V + v] == cnt;
                const double m = fabs(s);
                env = (m > env ? att : rel) * (env - m) + m;
                ok_en = ok_en && he[n * V + v] == env;
                if (phase >= hs_samples) phase -= hs_samples;
                if (phase < 1.0) value = s;
                phase++;
                ok_sh = ok_sh && hs[n * V + v] == value;
            }
        }
        EXPECT(ok_zx && ok_zc && ok_en && ok_sh && crossings > 50);
        EXPECT(hs[(N - 1) * V] == x[0]);  // hold == 0 samples once, ever
        // an output that is not asked for leaves its stage's state alone
        const std::vector<double> env0 = fetch(a.envelope(), V), hp0 = fetch(a.holdPhase(), V), px0 = fetch(a.previousX(), V);
        const std::vector<int64_t> cnt0 = fetch(a.runningCount(), V);
        a.render(150, dx.get(), zx2.get(), nullptr, nullptr, nullptr);  // (sample 149 is not one of the zeros sample 776 is)
        EXPECT(same(env0, fetch(a.envelope(), V)) && same(hp0, fetch(a.holdPhase(), V)) && cnt0 == fetch(a.runningCount(), V));
        EXPECT(!same(px0, fetch(a.previousX(), V)));
        a.render(100, dx.get(), nullptr, nullptr, en2.get(), nullptr);
        EXPECT(!same(env0, fetch(a.envelope(), V)) && same(hp0, fetch(a.holdPhase(), V)));
        // the crossings as the trigger block of an envelope bank: no host array in between
        {
            maxiEnvGenBank e1(V), e2(V);
            for (maxiEnvGenBank *e : {&e1, &e2}) e->setup({0, 1, 0}, {3, 20}, {1, 1}, false, false);
            DeviceArray<double> o1(N * V), o2(N * V), trig(N * V);
            trig.upload(hz);
            e1.play(N, zx1.get(), true, o1.get());
            e2.play(N, trig.get(), true, o2.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> h1 = o1.download();
            double peak = 0;
            for (double y : h1) peak = y > peak ? y : peak;
            EXPECT(same(h1, o2.download()) && peak == 1.0);
        }
        // refused and held windows
        bool refused = false;
        try {
            b.setWindow(0);
        } catch (const std::exception &e) {
            refused = strstr(e.what(), "window") != nullptr;
        }
        EXPECT(refused && b.window == window);
        maxiAnalysisBank c(V, cap), d(V, cap);
        d.setWindow(std::vector<uint32_t>{131, 130, 4000000000u, 130, 130});
        c.render(N, dx.get(), nullptr, zc1.get(), nullptr, nullptr);
        d.render(N, dx.get(), nullptr, zc2.get(), nullptr, nullptr);
        EXPECT(same(zc1.download(), zc2.download()));
        EXPECT((fetch(d.overflow(), V) == std::vector<uint32_t>{1, 0, 1, 0, 0}) && (fetch(c.overflow(), V) == std::vector<uint32_t>(V, 0)));
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_analysis_smoke: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    printf("facade_analysis_smoke: ok\n");
    return 0;
}
