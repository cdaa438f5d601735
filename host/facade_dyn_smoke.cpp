// host/facade_dyn_smoke.cpp -- maxiDynamicsBank and maxiRMSBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference: a stream rendered in two blocks equals the same stream rendered in one (state is carried),
// samples no section rewrites come out as exact zeros, and the RMS of a constant c settles at c * sqrt((w - 1) / w): the reference
// subtracts tail(w) AFTER the push, so its running sum holds w - 1 squares.  Exit status 0 = all of it held.
//
//   facade_dyn_smoke
#include <math.h>
#include <stdio.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "facade_dyn_smoke: %s failed\n", #c);     \
            fails++;                                                  \
        }                                                             \
    } while (0)

int main() {
    try {
        maxigpu::check(mxg_settings(44100, 2, 512), "mxg_settings");
        const size_t V = 70, N = 600;
        std::vector<double> x(N * V);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) {
                const double saw = (double)((n * (7 + v)) % 200) / 100.0 - 1.0;      // [-1, 1)
                x[n * V + v] = saw * ((n / 150) % 2 ? 0.9 : 0.02) * (v == 3 ? 0.0 : 1.0);  // loud and quiet stretches; voice 3 silent
            }
        DeviceArray<double> dx(N * V), one(N * V), two(N * V), lvl(N * V);
        dx.upload(x);
        const std::vector<double> thr(V, -20.0), ratio(V, 4.0), knee(V, 6.0);

        maxiDynamicsBank a(V, 4096, 4096), b(V, 4096, 4096);
        for (maxiDynamicsBank *d : {&a, &b}) {
            d->setCompress(thr, ratio, knee);
            d->setAttackHigh(1);
            d->setReleaseHigh(20);
            d->setRMSWindowSize(2);
            d->setLookAhead(0.5);
            d->analyser[5] = maxiDynamicsBank::PEAK;  // one voice on the peak detector
            d->touch();
        }
        a.compress(N, dx.get(), one.get());
        b.play(250, dx.get(), dx.get(), two.get(), lvl.get());
        b.play(N - 250, dx.get() + 250 * V, dx.get() + 250 * V, two.get() + 250 * V, lvl.get() + 250 * V);
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> h1 = one.download(), h2 = two.download();
        size_t same = 0, zeros = 0, nan = 0;
        double peak_out = 0.0;
        for (size_t i = 0; i < N * V; i++) {
            same += h1[i] == h2[i] || (h1[i] != h1[i] && h2[i] != h2[i]);
            zeros += h1[i] == 0.0;
            nan += h1[i] != h1[i];
            if (fabs(h1[i]) > peak_out) peak_out = fabs(h1[i]);
        }
        EXPECT(same == N * V);
        EXPECT(nan == 0);
        EXPECT(zeros > N);         // the silent voice, and negative samples below the threshold
        EXPECT(zeros < N * V);
        for (size_t n = 0; n < N; n++) EXPECT(h1[n * V + 3] == 0.0);
        EXPECT(peak_out > 0.0);
        std::vector<uint32_t> ovf(V, 1);
        maxigpu::check(mxg_memcpy_d2h(ovf.data(), a.overflow(), V * sizeof(uint32_t), nullptr), "mxg_memcpy_d2h");
        for (size_t v = 0; v < V; v++) EXPECT(ovf[v] == 0);

        const size_t cap = 64, M = 200;
        maxiRMSBank r(V, cap);
        r.setWindowSize(1.0);  // 44 samples
        std::vector<double> c(M * V, 0.5);
        DeviceArray<double> dc(M * V), ro(M * V);
        dc.upload(c);
        r.play(M, dc.get(), ro.get());
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> hr = ro.download();
        EXPECT(hr[(M - 1) * V] == sqrt(10.75 / 44.0));  // 43 squares of 0.5 over a window of 44: exact in double
        EXPECT(hr[0] > 0.0 && hr[0] < 0.5);  // the window is not full yet
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_dyn_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_dyn_smoke OK\n");
    return 0;
}
