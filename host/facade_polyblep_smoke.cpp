// host/facade_polyblep_smoke.cpp -- maxiPolyBLEPBank of include/maximilian_bank.hpp from plain C++ (no HIP headers), against the
// C-ABI calls.  Checks what needs no reference: for every waveform a bank rendered in uneven blocks -- a sync on a block edge and
// a pulse-width change in between -- equals mxg_polyblep_render called directly on the same blocks, bit for bit, phases
// included; per-sample frequencies that are constant over the block equal the per-voice form; the phase and the ten arithmetic
// waveforms equal mxg_polyblep_host (the same arithmetic on the CPU) bit for bit and the four sine waveforms stay within 2^-50
// of it; a bank without a pulse width equals one with 0.5; a bad waveform and a wrong vector length are refused.
// Exit status 0 = all of it held.
//
//   facade_polyblep_smoke
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
            fprintf(stderr, "facade_polyblep_smoke: %s failed\n", #c);     \
            fails++;                                                       \
        }                                                                  \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}

static bool is_sine(int wf) {
    return wf == MXG_PBLEP_SINE || wf == MXG_PBLEP_COSINE || wf == MXG_PBLEP_HALF_WAVE_RECTIFIED_SINE || wf == MXG_PBLEP_FULL_WAVE_RECTIFIED_SINE;
}

int main() {
    try {
        const double sr = 1000.0;
        maxiSettings::setup(1000, 2, 512);
        const size_t V = 7, N = 333, E = N * V;
        const size_t cuts[] = {0, 1, 9, 143, 144, N};
        const std::vector<double> freq = {0.0, -37.5, 61.625, 249.875, 7.25, 180.5, 117.3}, pw1 = {0.0, 0.00005, 0.3, 0.5, 0.99995, 1.0, 0.7},
                                  pw2 = {1.0, 0.3, 0.0, 0.99995, 0.5, 0.00005, 0.2}, phases = {2.75, -0.25, -3.0, 0.5, 0.0, 0.125, -1.5};
        std::vector<double> fblock(E);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) fblock[n * V + v] = v == 2 ? 250.0 + 60.0 * sin(0.07 * (double)n) : freq[v] * (1.0 + 0.3 * sin(0.05 * (double)n + v));
        DeviceArray<double> d_freq(V), d_fblock(E), d_pw(V), d_t(V), o1(E), o2(E);
        d_freq.upload(freq);
        d_fblock.upload(fblock);
        for (int wf = 0; wf < MXG_PBLEP_WAVEFORMS; wf++) {
            for (int ps = 0; ps < 2; ps++) {
                // the facade ...
                maxiPolyBLEPBank bank(V, sr);
                bank.set_waveform(wf);
                bank.set_pulse_width(pw1);
                // ... the C-ABI ...
                std::vector<double> t(V, 0.0), ht(V, 0.0), hout(E), hpw = pw1;
                d_t.upload(t);
                d_pw.upload(pw1);
                for (size_t b = 0; b + 1 < sizeof(cuts) / sizeof(cuts[0]); b++) {
                    const size_t a = cuts[b], n = cuts[b + 1] - a;
                    if (a == 143) {
                        bank.sync(phases);
                        for (size_t v = 0; v < V; v++) t[v] = ht[v] = maxiPolyBLEPBank::wrap(phases[v]);
                        maxigpu::check(mxg_sync(), "mxg_sync");
                        d_t.upload(t);
                    }
                    if (a == 144) {
                        bank.set_pulse_width(pw2);
                        maxigpu::check(mxg_sync(), "mxg_sync");
                        d_pw.upload(pw2);
                        hpw = pw2;
                    }
                    const double *f = ps ? d_fblock.get() + a * V : d_freq.get();
                    bank.render(n, f, ps != 0, o1.get() + a * V);
                    maxigpu::check(mxg_polyblep_render(wf, V, n, f, ps, d_pw.get(), sr, d_t.get(), o2.get() + a * V, nullptr), "mxg_polyblep_render");
                    // ... and the host entry point
                    maxigpu::check(mxg_polyblep_host(wf, V, n, ps ? fblock.data() + a * V : freq.data(), ps, hpw.data(), sr, ht.data(), hout.data() + a * V),
                                   "mxg_polyblep_host");
                }
                maxigpu::check(mxg_sync(), "mxg_sync");
                const std::vector<double> h1 = o1.download(), h2 = o2.download();
                std::vector<double> t1(V), t2 = d_t.download();
                maxigpu::check(mxg_memcpy_d2h(t1.data(), bank.phases(), V * sizeof(double), nullptr), "mxg_memcpy_d2h");
                EXPECT(same(h1, h2) && same(t1, t2));
                EXPECT(same(t1, ht));
                bool ok = true, moves = false;
                for (size_t i = 0; i < E; i++) {
                    const bool fb = ps && (fblock[i] / sr) * sr >= sr / 4;
                    if (is_sine(wf) || fb) ok = ok && fabs(h1[i] - hout[i]) <= ldexp(1.0, -50);
                    else ok = ok && !memcmp(&h1[i], &hout[i], sizeof(double));
                    moves = moves || h1[i] != h1[0];
                }
                if (!ok) fprintf(stderr, "facade_polyblep_smoke: waveform %d ps %d differs from the host arithmetic\n", wf, ps);
                EXPECT(ok && moves);
            }
            // per-sample frequencies that do not move equal the per-voice form; no pulse width equals 0.5
            std::vector<double> flat(E);
            for (size_t i = 0; i < E; i++) flat[i] = freq[i % V];
            d_fblock.upload(flat);
            maxiPolyBLEPBank a(V, sr), b(V, sr);
            a.set_waveform(wf);
            b.set_waveform(wf);
            b.set_pulse_width(0.5);
            a.render(N, d_freq.get(), false, o1.get());
            b.render(N, d_fblock.get(), true, o2.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            EXPECT(same(o1.download(), o2.download()));
            d_fblock.upload(fblock);
        }
        maxiPolyBLEPBank bank(V, sr);
        bool refused = false;
        try { bank.set_waveform(14); } catch (const std::exception &) { refused = true; }
        EXPECT(refused);
        refused = false;
        try { bank.sync(std::vector<double>(V + 1, 0.0)); } catch (const std::exception &) { refused = true; }
        EXPECT(refused);
        EXPECT(mxg_polyblep_render(MXG_PBLEP_SAWTOOTH, 0, 4, d_freq.get(), 0, nullptr, sr, d_t.get(), o1.get(), nullptr) == MXG_ERR_INVALID);
        EXPECT(mxg_polyblep_render(MXG_PBLEP_SAWTOOTH, V, 4, d_freq.get(), 0, nullptr, 0.0, d_t.get(), o1.get(), nullptr) == MXG_ERR_INVALID);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_polyblep_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_polyblep_smoke: ok\n");
    return 0;
}
