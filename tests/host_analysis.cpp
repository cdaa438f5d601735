// tests/host_analysis.cpp -- host build of mxg_analysis.h (tests/test_analysis_host.py; pinned to tests/golden/analysis.npz).
// ana_host_render takes the arguments of mxg_analysis_render (include/maxigpu.h) without the stream, plus the sample rate, on
// host arrays in the same layouts, and runs the step functions a lane of analysis.hip's kernel runs, voice after voice.
// With -DANA_HOST_MAIN the file is a stand-alone program that plays every stage over ring sizes and windows on both sides of
// the word edges, in blocks of uneven lengths (the sanitizer run).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mxg_analysis.h"

using namespace mxg;

extern "C" {

int ana_host_render(double sr, size_t V, size_t N, const double *in, int want, double *prev_x, const uint32_t *window, uint64_t *zring,
                    size_t cap, int32_t *zpos, int64_t *zcount, uint32_t *overflow, const double *attack, const double *release,
                    double *env, const double *hold_ms, int hold_ps, double *sah_phase, double *sah_value, double *o_zx, double *o_zcr,
                    double *o_env, double *o_sah) {
    const bool w_zcr = (want & MXG_ANA_WANT_ZCR) != 0, w_zx = (want & (MXG_ANA_WANT_ZX | MXG_ANA_WANT_ZCR)) != 0;
    const bool w_env = (want & MXG_ANA_WANT_ENV) != 0, w_sah = (want & MXG_ANA_WANT_SAH) != 0;
    for (size_t v = 0; v < V; v++) {
        double prev = w_zx ? prev_x[v] : 0.0;
        AnaZcr z = {nullptr, V, 1, 1, 0, 0, 0, 0, 0, -1, true};
        uint32_t over = 0;
        if (w_zcr) {
            z.ring = zring + v;
            z.cap = (int)cap;
            uint32_t w = window[v];
            if (w > (uint32_t)cap) { w = (uint32_t)cap; over = 1; }
            z.window = (int)w;
            z.idx = (zpos[v] >= 0 && zpos[v] < (int)cap) ? zpos[v] : 0;
            z.count = zcount[v];
            ana_zcr_open(z);
        }
        double e = w_env ? env[v] : 0.0, ph = w_sah ? sah_phase[v] : 0.0, hv = w_sah ? sah_value[v] : 0.0;
        for (size_t n = 0; n < N; n++) {
            const double x = in[n * V + v];
            if (w_zx) {
                const bool bit = ana_zx(prev, x);
                if (want & MXG_ANA_WANT_ZX) o_zx[n * V + v] = bit ? 1.0 : 0.0;
                if (w_zcr) o_zcr[n * V + v] = ana_zcr_step(z, bit);
            }
            if (w_env) o_env[n * V + v] = ana_follow<double>(e, attack[v], release[v], x);
            if (w_sah) o_sah[n * V + v] = ana_sah(ph, hv, x, ana_hold_samples(hold_ms[hold_ps ? n * V + v : v], sr));
        }
        if (w_zx) prev_x[v] = prev;
        if (w_zcr) {
            ana_zcr_close(z);
            zpos[v] = z.idx;
            zcount[v] = z.count;
            if (overflow) overflow[v] += over;
        }
        if (w_env) env[v] = e;
        if (w_sah) {
            sah_phase[v] = ph;
            sah_value[v] = hv;
        }
    }
    return 0;
}

// maxiEnvelopeFollowerF's recurrence in float
float ana_host_follow_f(float *env, float attack, float release, float x) { return ana_follow<float>(*env, attack, release, x); }

}  // extern "C"

#ifdef ANA_HOST_MAIN
int main() {
    unsigned long long acc = 0;
    const size_t caps[] = {1, 2, 63, 64, 65, 130, 1000};
    for (size_t cap : caps) {
        const uint32_t wins[] = {1, (uint32_t)cap, (uint32_t)(cap > 1 ? cap - 1 : 1), (uint32_t)(cap / 2 + 1), (uint32_t)cap + 5};
        for (uint32_t win : wins) {
            const size_t V = 3, nw = ana_ring_words(cap);
            std::vector<double> prev(V, 0.0), att(V, 0.9), rel(V, 0.99), env(V, 0.0), hold(V), ph(V, 0.0), hv(V, 0.0);
            std::vector<uint32_t> window(V, win), ovf(V, 0);
            std::vector<uint64_t> ring(nw * V, 0);
            std::vector<int32_t> pos(V);
            std::vector<int64_t> cnt(V, 0);
            for (size_t v = 0; v < V; v++) {
                pos[v] = v == 0 ? (int32_t)cap - 1 : (v == 1 ? (int32_t)(cap / 2) : (int32_t)cap + 7);  // the last: outside the ring
                hold[v] = v == 0 ? 0.0 : (v == 1 ? 2.5 : -3.0);
            }
            size_t t = 0;
            for (size_t N : {1, 7, 64, 2 * (int)cap + 5}) {
                std::vector<double> x(N * V), o(4 * N * V);
                for (size_t i = 0; i < N * V; i++, t++) x[i] = (double)((long)((t * 2654435761u) % 2001) - 1000) / 1000.0;
                ana_host_render(1000.0, V, N, x.data(), MXG_ANA_WANT_ALL, prev.data(), window.data(), ring.data(), cap, pos.data(),
                                cnt.data(), ovf.data(), att.data(), rel.data(), env.data(), hold.data(), 0, ph.data(), hv.data(),
                                o.data(), o.data() + N * V, o.data() + 2 * N * V, o.data() + 3 * N * V);
                ana_host_render(1000.0, V, N, x.data(), MXG_ANA_WANT_ZX | MXG_ANA_WANT_SAH, prev.data(), nullptr, nullptr, 0, nullptr,
                                nullptr, nullptr, nullptr, nullptr, nullptr, x.data(), 1, ph.data(), hv.data(), o.data(), nullptr, nullptr,
                                o.data() + 3 * N * V);
                for (size_t i = N * V; i < 2 * N * V; i++) acc += (unsigned long long)(o[i] < 0 ? -o[i] : o[i]);
            }
        }
    }
    float ef = 0.0f;
    for (int i = 0; i < 100; i++) acc += (unsigned long long)(1000.0f * ana_host_follow_f(&ef, 0.5f, 0.9f, (float)(i % 7) - 3.0f));
    printf("host_analysis: ok (%llu)\n", acc);
    return 0;
}
#endif
