// host/facade_revnet_smoke.cpp -- maxiReverbNetBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference: the layout of a hand-computed topology, a stream rendered in uneven blocks equals the same
// stream rendered in one (state is carried), an impulse comes back through a plain comb after its length with its feedback, a
// silent voice stays silent, clear() gives a fresh bank, and a topology the kernel does not take throws.  Then it prints a
// checksum of one fixed case (integer-made inputs and parameters), which tests/test_gpu_revnet.py compares with the Python bank's.
// Exit status 0 = all of it held.
//
//   facade_revnet_smoke
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "facade_revnet_smoke: %s failed\n", #c);     \
            fails++;                                                     \
        }                                                                \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main() {
    try {
        maxigpu::check(mxg_settings(44100, 2, 512), "mxg_settings");
        const size_t V = 21, N = 700;
        const std::vector<uint32_t> combs = {778, 64, 7}, lowp = {0, 1, 0}, aps = {125, 12};
        // the fixed case: everything below is exact in binary
        std::vector<double> x(N * V), cfb(V * 3), cut(V * 3), afb(V * 2);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) x[n * V + v] = v == 3 ? 0.0 : (double)((n * (7 + v)) % 200) / 128.0 - 0.75;
        for (size_t v = 0; v < V; v++) {
            for (size_t c = 0; c < 3; c++) {
                cfb[v * 3 + c] = 0.5 + (double)v / 64.0 - (double)c / 8.0;
                cut[v * 3 + c] = (double)(v % 8) / 8.0;
            }
            for (size_t a = 0; a < 2; a++) afb[v * 2 + a] = 0.25 + (double)v / 32.0 - (double)a / 2.0;
        }
        DeviceArray<double> dx(N * V), one(N * V), two(N * V);
        dx.upload(x);

        maxiReverbNetBank a(V, combs, aps, lowp), b(V, combs, aps, lowp);
        EXPECT(a.combs() == 3 && a.allpasses() == 2 && a.ringDoubles() == 986);
        const uint32_t off[5] = {0, 778, 842, 849, 974};
        for (int f = 0; f < 5; f++) EXPECT(a.offsets()[f] == off[f]);
        for (maxiReverbNetBank *k : {&a, &b}) {
            k->setCombFb(cfb);
            k->setCombCut(cut);
            k->setApFb(afb);
        }
        a.play(N, dx.get(), one.get());
        const size_t cuts[] = {0, 1, 64, 129, 130, 450, N};
        for (size_t k = 0; k + 1 < sizeof(cuts) / sizeof(cuts[0]); k++)
            b.play(cuts[k + 1] - cuts[k], dx.get() + cuts[k] * V, two.get() + cuts[k] * V);
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> h1 = one.download(), h2 = two.download();
        EXPECT(same(h1, h2));
        for (size_t n = 0; n < N; n++) EXPECT(h1[n * V + 3] == 0.0);

        // an impulse through one plain comb: x, then fb * x after its length
        maxiReverbNetBank c(V, {100}, {}, {}, 0.5);
        std::vector<double> imp(N * V, 0.0);
        for (size_t v = 0; v < V; v++) imp[v] = 1.0 + (double)v;
        dx.upload(imp);
        c.play(N, dx.get(), one.get());
        maxigpu::check(mxg_sync(), "mxg_sync");
        std::vector<double> h3 = one.download();
        for (size_t v = 0; v < V; v++) {
            EXPECT(h3[v] == imp[v] && h3[100 * V + v] == 0.5 * imp[v] && h3[200 * V + v] == 0.25 * imp[v]);
            EXPECT(h3[99 * V + v] == 0.0 && h3[101 * V + v] == 0.0);
        }
        c.clear();
        c.play(N, dx.get(), two.get());
        maxigpu::check(mxg_sync(), "mxg_sync");
        EXPECT(same(h3, two.download()));

        for (int which = 0; which < 3; which++) {
            bool threw = false;
            try {
                if (which == 0) maxiReverbNetBank bad(1, {}, {});
                else if (which == 1) maxiReverbNetBank bad(1, {63}, {5}, {1});
                else maxiReverbNetBank bad(1, {44101}, {});
            } catch (const std::exception &) {
                threw = true;
            }
            EXPECT(threw);
        }

        uint64_t h = 1469598103934665603ull;
        for (double s : h1) {
            uint64_t bits;
            memcpy(&bits, &s, 8);
            h = (h * 1099511628211ull) ^ bits;
        }
        printf("checksum %016" PRIx64 "\n", h);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_revnet_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_revnet_smoke OK\n");
    return 0;
}
