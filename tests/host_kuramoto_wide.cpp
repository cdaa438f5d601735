// tests/host_kuramoto_wide.cpp -- host build of mxg_kuramoto.h for sets of up to MXG_KURA_WIDE_MAX_N oscillators
// (tests/test_kuramoto_wide_host.py; compared with tests/golden/kuramoto_wide.npz).  kura_wide_host_render takes the arguments of
// mxg_kuramoto_wide_render (include/maxigpu.h) without the stream, plus the sample rate, on host arrays in the same layouts, and
// runs per set and sample what the lanes of kuramoto_wide.hip's kernel run: the same step functions in the same order, with the
// same choice between the trusted and the general sine, and the mean-field sum in the kernel's two steps (kura_meanfield_sums
// once per set, kura_meanfield_adj per oscillator).  It is tests/host_kuramoto.cpp's kura_host_render with std::vectors for the
// fixed arrays; for N <= 64 the two give the same bits.
// With -DKURA_WIDE_HOST_MAIN the file is a stand-alone program: every mode over set sizes on both sides of the wavefront counts
// in blocks of uneven lengths, with a stray and a NaN phase in the set's last wavefront (the sanitizer run).
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mxg_kuramoto.h"

using namespace mxg;

extern "C" {

int kura_wide_host_render(double sr, int mode, size_t S, size_t N_, size_t B, const double *freq, int freq_ps, const double *K, int K_ps,
                          double *phase, double *gathered, int32_t *update, int want, double *o_mix, double *o_phases) {
    const bool mf = (mode & MXG_KURA_MEANFIELD) != 0, async = (mode & MXG_KURA_ASYNC) != 0;
    if (N_ < 1 || N_ > MXG_KURA_WIDE_MAX_N) return -1;
    const int N = (int)N_;
    const double dt = MXG_TWOPI / sr;
    std::vector<double> g(N_), sg(N_), cg(N_), np(N_);
    for (size_t s = 0; s < S; s++) {
        double *ph = phase + s * N_;
        bool flag = true;
        double Ssum = 0.0, Csum = 0.0;
        if (async) {
            for (int j = 0; j < N; j++) g[j] = gathered[s * N_ + j];
            flag = update[s] != 0;
            if (mf && !flag) {
                for (int j = 0; j < N; j++) kura_sincos<false>(g[j], sg[j], cg[j]);
                kura_meanfield_sums(sg.data(), cg.data(), N, Ssum, Csum);
            }
        }
        for (size_t b = 0; b < B; b++) {
            const double fq = freq[freq_ps ? b * S + s : s], kk = K[K_ps ? b * S + s : s];
            const bool fl = !async || (b == 0 && flag);
            if (fl)
                for (int j = 0; j < N; j++) g[j] = ph[j];
            bool trusted = true;
            for (int j = 0; j < N; j++) trusted = trusted && fabs(ph[j]) <= kKuraTrust && fabs(g[j]) <= kKuraTrust;
            const double keff = fl ? kk : 0.0;
            if (mf && fl) {
                for (int j = 0; j < N; j++) kura_sincos<false>(g[j], sg[j], cg[j]);
                kura_meanfield_sums(sg.data(), cg.data(), N, Ssum, Csum);
            }
            for (int i = 0; i < N; i++) {
                double adj;
                if (mf) {
                    double si, ci;
                    kura_sincos<false>(ph[i], si, ci);
                    adj = kura_meanfield_adj(si, ci, Ssum, Csum);
                } else {
                    adj = trusted ? kura_adj_exact<true>(g.data(), N, ph[i]) : kura_adj_exact<false>(g.data(), N, ph[i]);
                }
                np[i] = kura_advance(ph[i], dt, fq, keff, N, adj);
            }
            for (int i = 0; i < N; i++) ph[i] = np[i];
            if (want & MXG_KURA_WANT_PHASES)
                for (int i = 0; i < N; i++) o_phases[(b * S + s) * N_ + i] = np[i];
            if (want & MXG_KURA_WANT_MIX) o_mix[b * S + s] = kura_mix(np.data(), N);
        }
        if (async && B > 0) {
            for (int j = 0; j < N; j++) gathered[s * N_ + j] = g[j];
            update[s] = 0;
        }
    }
    return 0;
}

}  // extern "C"

#ifdef KURA_WIDE_HOST_MAIN
int main() {
    double acc = 0.0;
    const size_t Ns[] = {1, 64, 65, 127, 128, 129, 200, 1023, 1024};
    for (int mode = 0; mode < 4; mode++) {
        for (size_t N : Ns) {
            const size_t S = N > 200 ? 2 : 3;
            std::vector<double> phase(S * N), gathered(S * N, 0.25), freq(S), K(S);
            std::vector<int32_t> update(S, 0);
            update[1] = 1;
            for (size_t i = 0; i < S * N; i++) phase[i] = fmod(0.37 + 1.618 * (double)i, MXG_TWOPI);
            for (size_t s = 0; s < S; s++) {
                freq[s] = s == 1 ? -3.0 : 2.0;
                K[s] = s == 0 ? -5.0 : 40.0;
            }
            size_t t = 0;
            const std::vector<size_t> blocks = N > 200 ? std::vector<size_t>{1, 3, 2} : std::vector<size_t>{1, 7, 16, 5};
            for (size_t bi = 0; bi < blocks.size(); bi++) {
                const size_t B = blocks[bi];
                std::vector<double> mix(B * S), po(B * S * N), fps(B * S), kps(B * S);
                for (size_t i = 0; i < B * S; i++, t++) {
                    fps[i] = 1.0 + 0.01 * (double)(t % 97);
                    kps[i] = (double)(t % 13) - 6.0;
                }
                int r = kura_wide_host_render(1000.0, mode, S, N, B, freq.data(), 0, K.data(), 0, phase.data(), gathered.data(), update.data(),
                                              3, mix.data(), po.data());
                r |= kura_wide_host_render(1000.0, mode, S, N, B, fps.data(), 1, kps.data(), 1, phase.data(), gathered.data(), update.data(), 1,
                                           mix.data(), nullptr);
                r |= kura_wide_host_render(1000.0, mode, S, N, B, freq.data(), 0, kps.data(), 1, phase.data(), gathered.data(), update.data(), 2,
                                           nullptr, po.data());
                if (r) {
                    printf("host_kuramoto_wide: a render was refused (mode %d, N %zu)\n", mode, N);
                    return 1;
                }
                if (bi + 2 == blocks.size()) {  // a stray phase in the set's last wavefront (the general sine), then a NaN there
                    phase[N - 1] = 1000.0;
                    update[0] = 1;
                }
                if (bi + 1 == blocks.size()) {
                    phase[N - 1] = NAN;
                    update[0] = 1;
                    kura_wide_host_render(1000.0, mode, S, N, 2, freq.data(), 0, K.data(), 0, phase.data(), gathered.data(), update.data(), 3,
                                          mix.data(), po.data());
                    if (!(mix[S] != mix[S])) {
                        printf("host_kuramoto_wide: a NaN phase did not reach the mix (mode %d, N %zu)\n", mode, N);
                        return 1;
                    }
                }
                acc += mix[0] == mix[0] ? mix[0] : 0.0;
            }
        }
    }
    std::vector<double> one(1, 0.0);
    if (kura_wide_host_render(1000.0, 0, 1, 0, 1, one.data(), 0, one.data(), 0, one.data(), nullptr, nullptr, 0, nullptr, nullptr) == 0 ||
        kura_wide_host_render(1000.0, 0, 1, 1025, 1, one.data(), 0, one.data(), 0, one.data(), nullptr, nullptr, 0, nullptr, nullptr) == 0) {
        printf("host_kuramoto_wide: a set of 0 or of 1025 oscillators was not refused\n");
        return 1;
    }
    printf("host_kuramoto_wide: ok (%.6f)\n", acc);
    return 0;
}
#endif
