// host/facade_reverb_smoke.cpp -- the reverb banks of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference: a stream rendered in uneven blocks equals the same stream rendered in one (state is carried),
// the first sample of an impulse is the comb sum through the allpass chain's direct path (4 or 8 combs, gain -0.85 a stage), the
// echo of the shortest ring arrives on its sample, the stereo bank's right channel is alive, and voices do not touch each other.
// Exit status 0 = all of it held.
//
//   facade_reverb_smoke
#include <stdio.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "facade_reverb_smoke: %s failed\n", #c);     \
            fails++;                                                     \
        }                                                                \
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
        const size_t V = 21, N = 1500;
        std::vector<double> x(N * V, 0.0);
        for (size_t v = 0; v < V; v++) x[v] = v == 3 ? 0.0 : 1.0 + (double)v;  // an impulse per voice; voice 3 silent
        for (size_t n = 700; n < 900; n++)
            for (size_t v = 0; v < V; v++) x[n * V + v] = v == 3 ? 0.0 : (double)((n * (7 + v)) % 200) / 100.0 - 1.0;
        DeviceArray<double> dx(N * V), one(2 * N * V), two(2 * N * V);
        dx.upload(x);
        const size_t cuts[] = {0, 1, 64, 129, 700, 1213, N};

        {  // maxiSatReverb
            maxiSatReverbBank a(V), b(V);
            EXPECT(a.combs() == 4 && a.allpasses() == 3 && a.ringDoubles() == 3992);
            a.play(N, dx.get(), one.get());
            for (size_t k = 0; k + 1 < sizeof(cuts) / sizeof(cuts[0]); k++)
                b.play(cuts[k + 1] - cuts[k], dx.get() + cuts[k] * V, two.get() + cuts[k] * V);
            maxigpu::check(mxg_sync(), "mxg_sync");
            std::vector<double> h1 = one.download(), h2 = two.download();
            h1.resize(N * V);
            h2.resize(N * V);
            EXPECT(same(h1, h2));
            for (size_t v = 0; v < V; v++) {
                const double imp = x[v];
                double t = 0.0;
                for (int c = 0; c < 4; c++) t += imp;
                for (int j = 0; j < 3; j++) t = t * (-0.85);
                EXPECT(h1[v] == t);
                EXPECT((h1[12 * V + v] != 0.0) == (v != 3));  // the 12-slot allpass answers on sample 12
                EXPECT(h1[5 * V + v] == 0.0);                  // ... and nothing before it
            }
            for (size_t n = 0; n < N; n++) EXPECT(h1[n * V + 3] == 0.0);
        }
        {  // maxiFreeVerb: play(x), and play(x, roomsize, absorbtion) in blocks
            maxiFreeVerbBank a(V), b(V);
            EXPECT(a.combs() == 8 && a.allpasses() == 31 && a.ringDoubles() == 18905);
            const std::vector<double> room(V, 0.5), absorb(V, 0.3);
            a.play(700, dx.get(), one.get());
            a.play(N - 700, dx.get() + 700 * V, room, absorb, one.get() + 700 * V);
            for (size_t k = 0; k + 1 < sizeof(cuts) / sizeof(cuts[0]); k++) {
                const size_t n0 = cuts[k], n = cuts[k + 1] - cuts[k];
                if (n0 < 700) b.play(n, dx.get() + n0 * V, two.get() + n0 * V);
                else b.play(n, dx.get() + n0 * V, room, absorb, two.get() + n0 * V);
            }
            maxigpu::check(mxg_sync(), "mxg_sync");
            std::vector<double> h1 = one.download(), h2 = two.download();
            h1.resize(N * V);
            h2.resize(N * V);
            EXPECT(same(h1, h2));
            for (size_t v = 0; v < V; v++) {
                double t = 0.0;
                for (int c = 0; c < 8; c++) t += x[v];
                for (int j = 0; j < 4; j++) t = t * (-0.85);
                EXPECT(h1[v] == t);
            }
            std::vector<double> wc(2 * V);
            maxigpu::check(mxg_memcpy_d2h(wc.data(), a.weightAndCutoff(), wc.size() * sizeof(double), nullptr), "mxg_memcpy_d2h");
            EXPECT(wc[0] == (0.5 * 0.10) + 0.84 && wc[1] == 0.3);
            for (size_t n = 0; n < N; n++) EXPECT(h1[n * V + 3] == 0.0);
        }
        {  // maxiFreeVerbStereo
            maxiFreeVerbStereoBank a(V), b(V);
            EXPECT(a.combs() == 8 && a.allpasses() == 4 && a.ringDoubles() == 12587);
            a.playStereo(N, dx.get(), one.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> h1 = one.download();
            size_t right = 0;
            for (size_t i = N * V; i < 2 * N * V; i++) right += h1[i] != 0.0;
            EXPECT(right > 100);          // the second step over the left channel's rings
            EXPECT(h1[N * V] == 0.0);     // ... which holds nothing on the first sample
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_reverb_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_reverb_smoke OK\n");
    return 0;
}
