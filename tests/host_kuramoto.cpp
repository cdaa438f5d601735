// tests/host_kuramoto.cpp -- host build of mxg_kuramoto.h (tests/test_kuramoto_host.py; compared with tests/golden/kuramoto.npz).
// kura_host_render takes the arguments of mxg_kuramoto_render (include/maxigpu.h) without the stream, plus the sample rate, on
// host arrays in the same layouts, and runs per set and sample what the lanes of kuramoto.hip's kernel run: the same step
// functions in the same order, with the same choice between the trusted and the general sine.
// With -DKURA_HOST_MAIN the file is a stand-alone program: every mode over set sizes on both sides of the segment widths in
// blocks of uneven lengths, with a stray and a NaN phase (the sanitizer run), and the error of kura_sin / kura_cos against long
// double over (-2 pi, 2 pi), the zeros' neighbourhoods included.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mxg_kuramoto.h"

using namespace mxg;

extern "C" {

int kura_host_render(double sr, int mode, size_t S, size_t N_, size_t B, const double *freq, int freq_ps, const double *K, int K_ps,
                     double *phase, double *gathered, int32_t *update, int want, double *o_mix, double *o_phases) {
    const bool mf = (mode & MXG_KURA_MEANFIELD) != 0, async = (mode & MXG_KURA_ASYNC) != 0;
    const int N = (int)N_;
    if (N < 1 || N > MXG_KURA_MAX_N) return -1;
    const double dt = MXG_TWOPI / sr;
    for (size_t s = 0; s < S; s++) {
        double *ph = phase + s * N_;
        double g[MXG_KURA_MAX_N], sg[MXG_KURA_MAX_N], cg[MXG_KURA_MAX_N], np[MXG_KURA_MAX_N];
        bool flag = true;
        if (async) {
            for (int j = 0; j < N; j++) g[j] = gathered[s * N_ + j];
            flag = update[s] != 0;
            if (mf && !flag)
                for (int j = 0; j < N; j++) kura_sincos<false>(g[j], sg[j], cg[j]);
        }
        for (size_t b = 0; b < B; b++) {
            const double fq = freq[freq_ps ? b * S + s : s], kk = K[K_ps ? b * S + s : s];
            const bool fl = !async || (b == 0 && flag);
            if (fl)
                for (int j = 0; j < N; j++) g[j] = ph[j];
            bool trusted = true;
            for (int j = 0; j < N; j++) trusted = trusted && fabs(ph[j]) <= kKuraTrust && fabs(g[j]) <= kKuraTrust;
            const double keff = fl ? kk : 0.0;
            if (mf && fl)
                for (int j = 0; j < N; j++) kura_sincos<false>(g[j], sg[j], cg[j]);
            for (int i = 0; i < N; i++) {
                double adj;
                if (mf) {
                    double si, ci;
                    kura_sincos<false>(ph[i], si, ci);
                    adj = kura_adj_meanfield(sg, cg, N, si, ci);
                } else {
                    adj = trusted ? kura_adj_exact<true>(g, N, ph[i]) : kura_adj_exact<false>(g, N, ph[i]);
                }
                np[i] = kura_advance(ph[i], dt, fq, keff, N, adj);
            }
            for (int i = 0; i < N; i++) ph[i] = np[i];
            if (want & MXG_KURA_WANT_PHASES)
                for (int i = 0; i < N; i++) o_phases[(b * S + s) * N_ + i] = np[i];
            if (want & MXG_KURA_WANT_MIX) o_mix[b * S + s] = kura_mix(np, N);
        }
        if (async && B > 0) {
            for (int j = 0; j < N; j++) gathered[s * N_ + j] = g[j];
            update[s] = 0;
        }
    }
    return 0;
}

double kura_host_sin(double x) { return kura_sin(x); }
double kura_host_cos(double x) { return kura_cos(x); }

// the largest error of kura_sin and kura_cos in ULPs of the result, against long double, over n arguments in (-2 pi, 2 pi) and
// the doubles around every multiple of pi / 2 in it
double kura_host_sin_error(size_t n) {
    double worst = 0.0;
    auto one = [&](double x) {
        const long double es = sinl((long double)x), ec = cosl((long double)x);
        const double s = kura_sin(x), c = kura_cos(x);
        int e;
        frexp((double)es, &e);
        const double us = (double)fabsl(((long double)s - es) / ldexpl(1.0L, e - 53));
        frexp((double)ec, &e);
        const double uc = (double)fabsl(((long double)c - ec) / ldexpl(1.0L, e - 53));
        if (es != 0.0L && us > worst) worst = us;
        if (ec != 0.0L && uc > worst) worst = uc;
    };
    uint64_t r = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < n; i++) {
        r = r * 6364136223846793005ull + 1442695040888963407ull;
        one(((double)(r >> 11) / 9007199254740992.0 * 2.0 - 1.0) * MXG_TWOPI);
    }
    for (int k = -4; k <= 4; k++) {
        double x = (double)k * 1.5707963267948966;
        double lo = x, hi = x;
        for (int i = 0; i < 200; i++) {
            one(lo);
            one(hi);
            lo = nextafter(lo, -100.0);
            hi = nextafter(hi, 100.0);
        }
        for (int q = 1; q < 60; q++) {
            one(x + ldexp(1.0, -q));
            one(x - ldexp(1.0, -q));
        }
    }
    return worst;
}

}  // extern "C"

#ifdef KURA_HOST_MAIN
int main() {
    double acc = 0.0;
    const size_t Ns[] = {1, 2, 3, 5, 31, 32, 33, 63, 64};
    for (int mode = 0; mode < 4; mode++) {
        for (size_t N : Ns) {
            const size_t S = 3;
            std::vector<double> phase(S * N), gathered(S * N, 0.25), freq(S), K(S);
            std::vector<int32_t> update(S, 0);
            update[1] = 1;
            for (size_t i = 0; i < S * N; i++) phase[i] = fmod(0.37 + 1.618 * (double)i, MXG_TWOPI);
            for (size_t s = 0; s < S; s++) {
                freq[s] = s == 1 ? -3.0 : 2.0;
                K[s] = s == 2 ? -5.0 : 40.0;
            }
            size_t t = 0;
            for (size_t B : {1, 7, 64, 30}) {
                std::vector<double> mix(B * S), po(B * S * N), fps(B * S), kps(B * S);
                for (size_t i = 0; i < B * S; i++, t++) {
                    fps[i] = 1.0 + 0.01 * (double)(t % 97);
                    kps[i] = (double)(t % 13) - 6.0;
                }
                kura_host_render(1000.0, mode, S, N, B, freq.data(), 0, K.data(), 0, phase.data(), gathered.data(), update.data(), 3,
                                 mix.data(), po.data());
                kura_host_render(1000.0, mode, S, N, B, fps.data(), 1, kps.data(), 1, phase.data(), gathered.data(), update.data(), 1,
                                 mix.data(), nullptr);
                kura_host_render(1000.0, mode, S, N, B, freq.data(), 0, kps.data(), 1, phase.data(), gathered.data(), update.data(), 2,
                                 nullptr, po.data());
                if (B == 64) {  // a stray phase (the general sine), then a NaN
                    phase[0] = 1000.0;
                    update[0] = 1;
                }
                if (B == 30) {
                    phase[N - 1] = NAN;
                    update[0] = 1;
                    kura_host_render(1000.0, mode, S, N, 2, freq.data(), 0, K.data(), 0, phase.data(), gathered.data(), update.data(), 3,
                                     mix.data(), po.data());
                    if (!(mix[S] != mix[S])) {
                        printf("host_kuramoto: a NaN phase did not reach the mix (mode %d, N %zu)\n", mode, N);
                        return 1;
                    }
                }
                acc += mix[0] == mix[0] ? mix[0] : 0.0;
            }
        }
    }
    const double err = kura_host_sin_error(400000);
    printf("host_kuramoto: ok (%.6f), sine / cosine error %.4f ULP\n", acc, err);
    return err < 0.85 ? 0 : 1;
}
#endif
