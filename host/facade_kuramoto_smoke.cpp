// host/facade_kuramoto_smoke.cpp -- maxiKuramotoBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference:
//   * with K = 0 a set runs free: phase += dt * (freq + 0.0), one wrap, mix = the phases summed in order / N.  No sine takes
//     part, so the device's phases and mix are the bits of that loop written out here (sets of 1, 3, 33 and 64);
//   * a coupled run against the reference's recurrence written out here with the host's sin(): the device's sine is within 1 ULP
//     of it per term, which over 300 samples at K = 8 stays many orders below the 1e-11 allowed (measured on the host build of
//     the same arithmetic: below 1e-14);
//   * a stream rendered in uneven blocks equals the same stream rendered in one, state included;
//   * an output that is not asked for is not written; the mean-field mode stays within 1e-10 of the exact one;
//   * an asynchronous set plays K only on the first sample after setPhase, refreshes its gathered phases then and only then,
//     and clears its flag; its neighbour in the same wavefront does neither;
//   * sets of 0 and of 65 oscillators are refused.  Exit status 0 = all of it held.
//
//   facade_kuramoto_smoke
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
            fprintf(stderr, "facade_kuramoto_smoke: %s failed\n", #c);     \
            fails++;                                                       \
        }                                                                  \
    } while (0)

static const double kTwoPi = 6.283185307179586476925286766559;

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}
static double maxdiff(const std::vector<double> &a, const std::vector<double> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e300;
    for (size_t i = 0; i < a.size() && i < b.size(); i++) m = fmax(m, fabs(a[i] - b[i]));
    return m;
}

// the reference's recurrence for S sets of N, host sin(); phases [S][N] in/out, mix [B][S], out [B][S][N]
static void host_play(size_t S, size_t N, size_t B, double sr, const std::vector<double> &freq, const std::vector<double> &K,
                      std::vector<double> &phases, std::vector<double> &mix, std::vector<double> &out) {
    const double dt = kTwoPi / sr;
    mix.assign(B * S, 0.0);
    out.assign(B * S * N, 0.0);
    std::vector<double> g(N);
    for (size_t b = 0; b < B; b++)
        for (size_t s = 0; s < S; s++) {
            double *p = &phases[s * N];
            for (size_t j = 0; j < N; j++) g[j] = p[j];
            double m = 0.0;
            for (size_t i = 0; i < N; i++) {
                double adj = 0;
                for (size_t j = 0; j < N; j++) adj += sin(g[j] - p[i]);
                p[i] += dt * (freq[s] + ((K[s] / (double)N) * adj));
                if (p[i] >= kTwoPi) p[i] -= kTwoPi;
                else if (p[i] < 0) p[i] += kTwoPi;
                m += p[i];
                out[(b * S + s) * N + i] = p[i];
            }
            mix[b * S + s] = m / (double)N;
        }
}

static std::vector<double> seeded(size_t n, unsigned seed) {
    std::vector<double> v(n);
    unsigned long long r = 0x9E3779B97F4A7C15ull + seed;
    for (size_t i = 0; i < n; i++) {
        r = r * 6364136223846793005ull + 1442695040888963407ull;
        v[i] = (double)(r >> 11) / 9007199254740992.0 * kTwoPi;
    }
    return v;
}

int main() {
    try {
        const double sr = 1000.0;
        maxiSettings::setup(1000, 2, 512);
        const size_t B = 300;
        for (size_t N : {1, 3, 33, 64}) {
            const size_t S = 5;
            std::vector<double> freq(S), K0(S, 0.0), K(S), p0 = seeded(S * N, (unsigned)N);
            for (size_t s = 0; s < S; s++) {
                freq[s] = s % 2 ? -3.5 - (double)s : 2.25 + (double)s;
                K[s] = s == 2 ? -1.0 : 8.0;
            }
            // free run: the bits of the loop
            {
                maxiKuramotoBank k(S, N);
                k.setFreq(freq);
                k.setK(K0);
                k.setPhases(p0);
                DeviceArray<double> mix(B * S), out(B * S * N);
                k.play(B, mix.get(), out.get());
                std::vector<double> hp = p0, hm, ho;
                host_play(S, N, B, sr, freq, K0, hp, hm, ho);
                maxigpu::check(mxg_sync(), "mxg_sync");
                EXPECT(same(mix.download(), hm));
                EXPECT(same(out.download(), ho));
                EXPECT(same(k.phases(), hp));
                bool wrapped = false;
                for (size_t i = S * N; i < ho.size(); i++) wrapped = wrapped || fabs(ho[i] - ho[i - S * N]) > 3.0;
                EXPECT(wrapped);
            }
            // coupled: within the sine's last place, accumulated
            maxiKuramotoBank a(S, N), b(S, N), mf(S, N, true);
            for (maxiKuramotoBank *k : {&a, &b, &mf}) {
                k->setFreq(freq);
                k->setK(K);
                k->setPhases(p0);
            }
            DeviceArray<double> mix1(B * S), out1(B * S * N), mix2(B * S), out2(B * S * N), mix3(B * S);
            a.play(B, mix1.get(), out1.get());
            std::vector<double> hp = p0, hm, ho;
            host_play(S, N, B, sr, freq, K, hp, hm, ho);
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> m1 = mix1.download(), o1 = out1.download();
            EXPECT(maxdiff(m1, hm) <= 1e-11);
            EXPECT(maxdiff(o1, ho) <= 1e-11);
            EXPECT(maxdiff(o1, std::vector<double>(o1.size(), 0.0)) > 1.0);
            // uneven blocks = one block
            const size_t cuts[] = {0, 1, 8, 9, 64, 130, 131, B};
            for (size_t c = 0; c + 1 < sizeof(cuts) / sizeof(cuts[0]); c++)
                b.play(cuts[c + 1] - cuts[c], mix2.get() + cuts[c] * S, out2.get() + cuts[c] * S * N);
            maxigpu::check(mxg_sync(), "mxg_sync");
            EXPECT(same(mix2.download(), m1) && same(out2.download(), o1) && same(a.phases(), b.phases()));
            // the mean-field mode, mix only: the phases block is not touched
            mf.play(B, mix3.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            EXPECT(maxdiff(mix3.download(), m1) <= 1e-10);
            EXPECT(maxdiff(mf.phases(), a.phases()) <= 1e-10);
        }
        // asynchronous: two sets of 3 share a wavefront; only set 0 is told something
        {
            const size_t S = 2, N = 3, Bq = 5;
            maxiKuramotoBank q(S, N, false, true);
            std::vector<double> p0 = {0.5, 2.0, 4.0, 1.0, 3.0, 5.0};
            q.setFreq(2.0);
            q.setK(40.0);
            q.setPhases(p0);  // raises both flags ...
            DeviceArray<double> out(Bq * S * N), mix(Bq * S);
            q.play(1, mix.get(), out.get());  // ... which this consumes
            maxigpu::check(mxg_sync(), "mxg_sync");
            std::vector<int32_t> up(S);
            maxigpu::check(mxg_memcpy_d2h(up.data(), q.update(), S * sizeof(int32_t), nullptr), "d2h");
            EXPECT(up[0] == 0 && up[1] == 0);
            std::vector<double> g(S * N);
            maxigpu::check(mxg_memcpy_d2h(g.data(), q.gathered(), S * N * sizeof(double), nullptr), "d2h");
            EXPECT(same(g, p0));
            const std::vector<double> p1 = q.phases();
            q.setPhase(1.25, 1, 0);
            maxigpu::check(mxg_memcpy_d2h(up.data(), q.update(), S * sizeof(int32_t), nullptr), "d2h");
            EXPECT(up[0] == 1 && up[1] == 0);
            q.play(Bq, mix.get(), out.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            maxigpu::check(mxg_memcpy_d2h(up.data(), q.update(), S * sizeof(int32_t), nullptr), "d2h");
            maxigpu::check(mxg_memcpy_d2h(g.data(), q.gathered(), S * N * sizeof(double), nullptr), "d2h");
            EXPECT(up[0] == 0 && up[1] == 0);
            EXPECT(g[0] == p1[0] && g[1] == 1.25 && g[2] == p1[2]);        // set 0 gathered what it was told
            EXPECT(g[3] == p0[3] && g[4] == p0[4] && g[5] == p0[5]);        // set 1 still holds the first gather
            // set 1 ran free for all Bq samples: the bits of phase += dt * (freq + 0.0)
            const std::vector<double> o = out.download();
            std::vector<double> p(p1.begin() + N, p1.end());
            bool free_run = true;
            for (size_t b = 0; b < Bq; b++)
                for (size_t i = 0; i < N; i++) {
                    p[i] += kTwoPi / sr * (2.0 + 0.0);
                    if (p[i] >= kTwoPi) p[i] -= kTwoPi;
                    free_run = free_run && o[(b * S + 1) * N + i] == p[i];
                }
            EXPECT(free_run);
            // set 0 felt K on the first sample only: afterwards each step is the free step
            bool coupled_once = fabs(o[0] - (p1[0] + kTwoPi / sr * 2.0)) > 1e-6;
            for (size_t b = 1; b < Bq; b++)
                for (size_t i = 0; i < N; i++) {
                    double e = o[((b - 1) * S) * N + i] + kTwoPi / sr * (2.0 + 0.0);
                    if (e >= kTwoPi) e -= kTwoPi;
                    coupled_once = coupled_once && o[(b * S) * N + i] == e;
                }
            EXPECT(coupled_once);
        }
        // refused without a launch
        for (size_t N : {0, 65}) {
            bool threw = false;
            try {
                maxiKuramotoBank bad(1, N);
            } catch (const std::exception &) {
                threw = true;
            }
            EXPECT(threw);
            DeviceArray<double> d(128);
            EXPECT(mxg_kuramoto_render(0, 1, N, 1, d.get(), 0, d.get(), 0, d.get(), nullptr, nullptr, MXG_KURA_WANT_MIX, d.get(), nullptr,
                                       nullptr) < 0);
        }
        maxiSettings::setup(44100, 2, 1024);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_kuramoto_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_kuramoto_smoke: ok\n");
    return 0;
}
