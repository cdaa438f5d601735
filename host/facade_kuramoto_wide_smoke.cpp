// host/facade_kuramoto_wide_smoke.cpp -- maxiKuramotoWideBank of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// A sync and an async bank of 3 sets of N = 200 oscillators (four wavefronts a set, the last one with 56 surplus lanes) are played
// in uneven blocks, with setPhase between blocks, beside a plain C++ loop over the step functions of
// maximilian_amd/csrc/mxg_kuramoto.h -- the kernel's own arithmetic, which g++ compiles to the same bits -- and must give its
// bits: mix, phases after every sample, and state.  The mean-field mode, played for its mix alone,
// stays within 1e-10 of the exact one; sets of 0 and of 1025 oscillators are refused.  Exit status 0 = all of it held.
//
//   facade_kuramoto_wide_smoke
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"
#include "mxg_kuramoto.h"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                               \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "facade_kuramoto_wide_smoke: %s failed\n", #c);     \
            fails++;                                                            \
        }                                                                       \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}
static double maxdiff(const std::vector<double> &a, const std::vector<double> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e300;
    for (size_t i = 0; i < a.size() && i < b.size(); i++) m = fmax(m, fabs(a[i] - b[i]));
    return m;
}

// The exact form for S sets of N over B samples, as the reference orders it: gather (async: only when told, and K = 0
// otherwise), every oscillator against the gathered phases, the mix over the new phases.  All phases stay in [0, 2 pi), so the
// trusted sine applies.  phases [S][N], gathered [S][N] and update [S] in/out; mix [B][S] and out [B][S][N] are appended to.
static void host_play(bool async, size_t S, size_t N, size_t B, double sr, const std::vector<double> &freq, const std::vector<double> &K,
                      std::vector<double> &phases, std::vector<double> &gathered, std::vector<int> &update, std::vector<double> &mix,
                      std::vector<double> &out) {
    const double dt = MXG_TWOPI / sr;
    const size_t at = mix.size() / S;
    mix.resize((at + B) * S);
    out.resize((at + B) * S * N);
    std::vector<double> np(N);
    for (size_t s = 0; s < S; s++) {
        double *p = &phases[s * N], *g = &gathered[s * N];
        for (size_t b = 0; b < B; b++) {
            const bool fl = !async || (b == 0 && update[s]);
            if (fl)
                for (size_t j = 0; j < N; j++) g[j] = p[j];
            for (size_t i = 0; i < N; i++)
                np[i] = mxg::kura_advance(p[i], dt, freq[s], fl ? K[s] : 0.0, (int)N, mxg::kura_adj_exact<true>(g, (int)N, p[i]));
            for (size_t i = 0; i < N; i++) out[((at + b) * S + s) * N + i] = p[i] = np[i];
            mix[(at + b) * S + s] = mxg::kura_mix(np.data(), (int)N);
        }
        update[s] = 0;
    }
}

static std::vector<double> seeded(size_t n, unsigned seed) {
    std::vector<double> v(n);
    unsigned long long r = 0x9E3779B97F4A7C15ull + seed;
    for (size_t i = 0; i < n; i++) {
        r = r * 6364136223846793005ull + 1442695040888963407ull;
        v[i] = (double)(r >> 11) / 9007199254740992.0 * MXG_TWOPI;
    }
    return v;
}

int main() {
    try {
        const double sr = 1000.0;
        maxiSettings::setup(1000, 2, 512);
        const size_t S = 3, N = 200, B = 40;
        const size_t cuts[] = {0, 1, 8, 9, 25, B};
        const size_t ncuts = sizeof(cuts) / sizeof(cuts[0]);
        std::vector<double> freq = {35.0, -28.0, 41.5}, K = {8.0, -3.0, 20.0};
        for (int async = 0; async < 2; async++) {
            maxiKuramotoWideBank k(S, N, false, async != 0), mf(S, N, true, async != 0);
            const std::vector<double> p0 = seeded(S * N, 7u + (unsigned)async);
            for (maxiKuramotoWideBank *q : {&k, &mf}) {
                q->setFreq(freq);
                q->setK(K);
                q->setPhases(p0);  // (async: raises every flag)
            }
            std::vector<double> hp = p0, hg(S * N, 0.0), hm, ho;
            std::vector<int> hu(S, async);
            DeviceArray<double> mix(B * S), out(B * S * N), mfmix(B * S);
            for (size_t c = 0; c + 1 < ncuts; c++) {
                if (c == 2) {  // setPhase between two blocks: oscillator 199 (the set's last wavefront) of set 1, oscillator 0 of set 2
                    for (maxiKuramotoWideBank *q : {&k, &mf}) {
                        q->setPhase(0.5, N - 1, 1);
                        q->setPhase(4.25, 0, 2);
                    }
                    hp[1 * N + N - 1] = 0.5;
                    hp[2 * N] = 4.25;
                    if (async) hu[1] = hu[2] = 1;
                }
                const size_t n = cuts[c + 1] - cuts[c];
                k.play(n, mix.get() + cuts[c] * S, out.get() + cuts[c] * S * N);
                mf.play(n, mfmix.get() + cuts[c] * S);
                host_play(async != 0, S, N, n, sr, freq, K, hp, hg, hu, hm, ho);
            }
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> m = mix.download();
            EXPECT(same(m, hm));
            EXPECT(same(out.download(), ho));
            EXPECT(same(k.phases(), hp));
            EXPECT(maxdiff(ho, std::vector<double>(ho.size(), 0.0)) > 1.0);
            bool wrapped = false;
            for (size_t i = S * N; i < ho.size(); i++) wrapped = wrapped || fabs(ho[i] - ho[i - S * N]) > 3.0;
            EXPECT(wrapped);
            if (async) {
                std::vector<double> g(S * N);
                std::vector<int32_t> up(S, 7);
                maxigpu::check(mxg_memcpy_d2h(g.data(), k.gathered(), S * N * sizeof(double), nullptr), "d2h");
                maxigpu::check(mxg_memcpy_d2h(up.data(), k.update(), S * sizeof(int32_t), nullptr), "d2h");
                EXPECT(same(g, hg));
                EXPECT(up[0] == 0 && up[1] == 0 && up[2] == 0);
                EXPECT(g[0] == p0[0] && g[1 * N + N - 1] == 0.5 && g[2 * N] == 4.25);  // set 0 gathered once; sets 1 and 2 when told
            }
            EXPECT(maxdiff(mfmix.download(), m) <= 1e-10);
            EXPECT(maxdiff(mf.phases(), k.phases()) <= 1e-10);
        }
        // refused without a launch
        for (size_t Nbad : {0, 1025}) {
            bool threw = false;
            try {
                maxiKuramotoWideBank bad(1, Nbad);
            } catch (const std::exception &) {
                threw = true;
            }
            EXPECT(threw);
            DeviceArray<double> d(128);
            EXPECT(mxg_kuramoto_wide_render(0, 1, Nbad, 1, d.get(), 0, d.get(), 0, d.get(), nullptr, nullptr, MXG_KURA_WANT_MIX, d.get(),
                                            nullptr, nullptr) < 0);
        }
        maxiSettings::setup(44100, 2, 1024);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_kuramoto_wide_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_kuramoto_wide_smoke: ok\n");
    return 0;
}
