// host/facade_dattaro_smoke.cpp -- maxiDattaroReverbBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference: the lengths at 44 100 and 22 050 Hz, a stream rendered in uneven blocks equals the same stream
// rendered in one (state is carried), an impulse reaches the right channel through D2's nearest tap after 1 221 samples and the
// left through D0's after 1 838 with the value the direct paths of the input allpasses give it, a silent voice stays silent, a
// bank at another sample rate answers at other times, and a sample rate outside the accepted range throws.
// Exit status 0 = all of it held.
//
//   facade_dattaro_smoke
#include <stdio.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "facade_dattaro_smoke: %s failed\n", #c);     \
            fails++;                                                      \
        }                                                                 \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!(a[i] == b[i])) return false;
    return true;
}

int main() {
    try {
        maxigpu::check(mxg_settings(44100, 2, 512), "mxg_settings");
        const size_t V = 21, N = 2600;
        std::vector<double> x(N * V, 0.0);
        for (size_t v = 0; v < V; v++) x[v] = v == 3 ? 0.0 : 1.0 + (double)v;  // an impulse per voice; voice 3 silent
        for (size_t n = 1900; n < 2100; n++)
            for (size_t v = 0; v < V; v++) x[n * V + v] = v == 3 ? 0.0 : (double)((n * (7 + v)) % 200) / 100.0 - 1.0;
        DeviceArray<double> dx(N * V), one(2 * N * V), two(2 * N * V);
        dx.upload(x);
        const size_t cuts[] = {0, 1, 64, 129, 700, 1213, 2000, N};

        maxiDattaroReverbBank a(V), b(V), half(V, 22050);
        EXPECT(a.sampleRate() == 44100 && a.ringDoubles() == 32312);
        const uint32_t len[10] = {210, 158, 1343, 3930, 994, 2663, 6240, 4680, 6589, 5505};
        for (int r = 0; r < 10; r++) EXPECT(a.lengths()[r] == len[r]);
        EXPECT(a.tapPositions()[8] == 5367 && a.tapRings()[8] == 8 && a.tapPositions()[1] == 4401 && a.tapRings()[1] == 6);
        EXPECT(half.lengths()[8] == 3294 && half.lengths()[1] == 79);
        a.playStereo(N, dx.get(), one.get());
        for (size_t k = 0; k + 1 < sizeof(cuts) / sizeof(cuts[0]); k++) {
            // the two channels of a block are N_block * V apart: render into a scratch pair and gather
            const size_t n0 = cuts[k], n = cuts[k + 1] - cuts[k];
            DeviceArray<double> blk(2 * n * V);
            b.playStereo(n, dx.get() + n0 * V, blk.get());
            maxigpu::check(mxg_memcpy_d2d_async(two.get() + n0 * V, blk.get(), n * V * sizeof(double), nullptr), "d2d");
            maxigpu::check(mxg_memcpy_d2d_async(two.get() + (N + n0) * V, blk.get() + n * V, n * V * sizeof(double), nullptr), "d2d");
            maxigpu::check(mxg_sync(), "mxg_sync");
        }
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> h1 = one.download(), h2 = two.download();
        EXPECT(same(h1, h2));
        for (size_t v = 0; v < V; v++) {
            double t = 0.8 * x[v];
            t = t * (-0.75);
            t = t * (-0.75);
            t = t * (-0.625);
            t = t * (-0.625);
            t = t * (-0.7);
            EXPECT(h1[(N + 1221) * V + v] == t);  // right: tap 8 of D2, 6589 - 1 - 5367 samples after the write
            EXPECT(h1[1838 * V + v] == t);        // left: tap 1 of D0, 6240 - 1 - 4401
            for (size_t n = 0; n < 1221; n++) EXPECT(h1[(N + n) * V + v] == 0.0);
            for (size_t n = 0; n < 1838; n++) EXPECT(h1[n * V + v] == 0.0);
        }
        for (size_t n = 0; n < 2 * N; n++) EXPECT(h1[n * V + 3] == 0.0);

        half.playStereo(N, dx.get(), one.get());
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> h3 = one.download();
        EXPECT(h3[(N + 610) * V] != 0.0 && h3[(N + 609) * V] == 0.0);  // 3294 - 1 - 2683

        bool threw = false;
        try {
            maxiDattaroReverbBank bad(1, 1000);
        } catch (const std::exception &) {
            threw = true;
        }
        EXPECT(threw);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_dattaro_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_dattaro_smoke OK\n");
    return 0;
}
