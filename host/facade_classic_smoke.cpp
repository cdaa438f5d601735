// host/facade_classic_smoke.cpp -- maxiDynBank, maxiEnvelopeBank, maxiLagExpBank and maxiMapBank of include/maximilian_bank.hpp
// from plain C++ (no HIP headers).  Checks what needs no reference: every bit-exact bank equals the library's host form of the
// same call (mxg_*_host: the shared arithmetic on host arrays), state included; a render in uneven blocks equals the render in
// one; compress() after the setters equals compressor() with the coefficients the host helpers give; the envelope's trigger
// block equals trigger() between blocks; a map in place equals the map into a second block; linexp, explin, ampToDbs and
// dbsToAmp stay within the bounds of DESIGN.md section 4 of the host libm's value (the absolute ones evaluated per element); bad arguments are refused by name.
// Exit status 0 = all of it held.
//
//   facade_classic_smoke
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "facade_classic_smoke: %s failed\n", #c);     \
            fails++;                                                      \
        }                                                                 \
    } while (0)

template <typename T>
static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

static double ulp(double y) { return nextafter(fabs(y), INFINITY) - fabs(y); }  // the spacing of the doubles at |y|

// The absolute bounds of DESIGN.md section 4, K23 (tests/classic_host.py: explin_bound, amptodbs_bound), per element, with the
// OpenCL ceiling of 3 ULP for log / log10 and 1 for the host libm: two logarithms of one operand are 4 ULP apart.
static double explin_bound(double l, double den, double span, double y) {  // l = log(val / inMin), y = the result
    const double a = fabs(l) / fabs(den), b = a * fabs(span);
    return 4 * ulp(l) / fabs(den) * fabs(span) + ulp(a) * fabs(span) + ulp(b) + ulp(y);
}
static double amptodbs_bound(double y) { return 4 * ulp(y / 20.0) * 20.0 + ulp(y); }  // y = log10(amp) * 20.0

static double ulps(double a, double b) {  // distance in ULPs of b
    if (a == b) return 0;
    int e;
    frexp(b, &e);
    return fabs(a - b) / ldexp(1.0, e - 53);
}

template <typename T>
static std::vector<T> fetch(const T *d, size_t n) {
    std::vector<T> h(n);
    maxigpu::check(mxg_sync(), "mxg_sync");
    maxigpu::check(mxg_memcpy_d2h(h.data(), d, n * sizeof(T), nullptr), "mxg_memcpy_d2h");
    return h;
}

int main() {
    try {
        maxiSettings::setup(44100, 2, 512);
        const size_t V = 6, N = 700, E = N * V;
        const size_t cuts[] = {0, 1, 8, 9, 64, 130, 131, 300, N};
        const size_t NC = sizeof(cuts) / sizeof(cuts[0]);
        std::vector<double> x(E), ref(E);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) {
                const double loud = (n % (150 + 20 * v)) < 60 ? 1.3 : 0.2;
                x[n * V + v] = loud * (2.0 * fmod((double)n * (0.013 + 0.002 * (double)v), 1.0) - 1.0);
            }
        DeviceArray<double> dx(E), o1(E), o2(E);
        dx.upload(x);

        // ---- maxiDyn: gate then compressor on one state, in one block and in uneven blocks, against the host form
        const std::vector<double> thr = {0.5, 0.4, 0.6, 0.5, 0.3, 5.0}, att = {0.5, 1.0, 0.01, 0.2, 0.3, 1.0}, rel = {0.99, 0.9995, 0.9, 0.995, 0.97, 0.9};
        const std::vector<double> ratio = {4.0, 0.75, 8.0, 2.5, 3.0, 1.0};
        const std::vector<int64_t> hold = {0, 1, 50, 30, 7, 1};
        {
            maxiDynBank a(V), b(V);
            a.gate(N, dx.get(), thr, hold, att, rel, o1.get());
            for (size_t k = 0; k + 1 < NC; k++) b.gate(cuts[k + 1] - cuts[k], dx.get() + cuts[k] * V, thr, hold, att, rel, o2.get() + cuts[k] * V);
            std::vector<double> dst(3 * V, 0.0);
            std::vector<int64_t> ist(4 * V, 0);
            maxigpu::check(mxg_dyn_gate_host(V, N, x.data(), thr.data(), att.data(), rel.data(), 0, hold.data(), dst.data(), ist.data(), ref.data()), "mxg_dyn_gate_host");
            EXPECT(same(o1.download(), ref) && same(o2.download(), ref));
            EXPECT(same(fetch(a.state(), 3 * V), dst) && same(fetch(b.state(), 3 * V), dst) && same(fetch(a.phases(), 4 * V), ist) && same(fetch(b.phases(), 4 * V), ist));
            bool opened = false, shut = true;
            for (size_t n = 0; n < N; n++) { opened = opened || ref[n * V] != 0.0; shut = shut && ref[n * V + 5] == 0.0; }
            EXPECT(opened && shut);  // voice 5 never passes its threshold
            std::vector<double> mk(V);
            for (size_t v = 0; v < V; v++) mk[v] = mxg_dyn_makeup_host(ratio[v]);
            EXPECT(mk[5] == 1.0 && mk[0] == 1 + log(4.0));
            a.compressor(N, dx.get(), ratio, thr, att, rel, o1.get());
            for (size_t k = 0; k + 1 < NC; k++) b.compressor(cuts[k + 1] - cuts[k], dx.get() + cuts[k] * V, ratio, thr, att, rel, o2.get() + cuts[k] * V);
            maxigpu::check(mxg_dyn_compress_host(V, N, x.data(), ratio.data(), mk.data(), thr.data(), att.data(), rel.data(), 0, dst.data(), ist.data(), ref.data()),
                           "mxg_dyn_compress_host");
            EXPECT(same(o1.download(), ref) && same(o2.download(), ref));
            EXPECT(same(fetch(a.state(), 3 * V), dst) && same(fetch(b.phases(), 4 * V), ist));
            // compress() after the setters = compressor() with the members
            maxiDynBank c(V), d(V);
            c.setRatio(3.0); c.setThreshold(0.45); c.setAttack(2.0); c.setRelease(1.5);
            c.compress(N, dx.get(), o1.get());
            d.compressor(N, dx.get(), 3.0, 0.45, mxg_dyn_coeff_host(2.0, 44100.0), mxg_dyn_coeff_host(1.5, 44100.0), o2.get());
            EXPECT(same(o1.download(), o2.download()) && mxg_dyn_coeff_host(2.0, 44100.0) == pow(0.01, 1.0 / (2.0 * 44100.0 * 0.001)));
        }

        // ---- maxiEnvelope: a trigger block against trigger() between blocks, against the host form
        {
            const double k = 44100 * 0.0011;  // a segment time of s / k lasts s samples
            const std::vector<double> segs = {1.0, 100 / k, 0.25, 150 / k, 0.75, 0.0, 0.5, 50 / k};
            std::vector<double> trig(E, 0.0);
            for (size_t v = 0; v < V; v++) trig[v] = 1.0;
            for (size_t v = 0; v < 3; v++) trig[400 * V + v] = -2.0;  // three voices again, in the middle of their tables
            DeviceArray<double> dt(E);
            dt.upload(trig);
            maxiEnvelopeBank a(V, segs), b(V, segs);
            a.line(N, dt.get(), 0, 0.0, o1.get());
            b.trigger(0, 0.0);
            b.line(400, o2.get());
            std::vector<int32_t> mask(V, 0);
            mask[0] = mask[1] = mask[2] = 1;
            b.trigger(std::vector<int32_t>(V, 0), std::vector<double>(V, 0.0), &mask);
            b.line(N - 400, o2.get() + 400 * V);
            std::vector<double> sv(8 * V), dst(2 * V, 0.0), amp(V, 0.0);
            for (size_t s = 0; s < 8; s++)
                for (size_t v = 0; v < V; v++) sv[s * V + v] = segs[s];
            std::vector<int32_t> count(V, 8), tix(V, 0), ist(2 * V, 0);
            maxigpu::check(mxg_envelope_line_host(V, N, 8, sv.data(), count.data(), trig.data(), tix.data(), amp.data(), dst.data(), ist.data(), ref.data()),
                           "mxg_envelope_line_host");
            EXPECT(same(o1.download(), ref) && same(o2.download(), ref));
            EXPECT(same(fetch(a.state(), 2 * V), dst) && same(fetch(b.state(), 2 * V), dst) && same(fetch(a.indices(), 2 * V), ist) && same(fetch(b.indices(), 2 * V), ist));
            EXPECT(fabs(ref[100 * V + 5] - 1.0) < 1e-9 && ref[50 * V + 5] > 0.4 && ref[50 * V + 5] < 0.6);  // the first segment lands on its target
            EXPECT(std::isnan(ref[(N - 1) * V + 5]) || std::isinf(ref[(N - 1) * V + 5]));                        // the zero segment time
            bool refused = false;
            try {
                a.trigger(7, 0.5);  // outside [0, count - 2]
            } catch (const std::exception &e) {
                refused = strstr(e.what(), "trigger index") != nullptr;
            }
            EXPECT(refused);
        }

        // ---- maxiLagExp: blocks, the desynchronised pair
        {
            maxiLagExpBank a(V, 0.25, 1.0), b(V, 0.25, 1.0);
            a.setAlpha(0.9);
            b.setAlpha(0.9);
            a.addSample(N, dx.get(), o1.get());
            for (size_t k = 0; k + 1 < NC; k++) b.addSample(cuts[k + 1] - cuts[k], dx.get() + cuts[k] * V, o2.get() + cuts[k] * V);
            std::vector<double> al(V, 0.9), rc(V, 0.75), val(V, 1.0);
            maxigpu::check(mxg_lag_host(V, N, x.data(), al.data(), rc.data(), 0, val.data(), ref.data()), "mxg_lag_host");
            EXPECT(same(o1.download(), ref) && same(o2.download(), ref) && same(a.value(), val) && same(b.value(), val));
            EXPECT(ref[0] == (0.9 * x[0]) + (0.75 * 1.0));
        }

        // ---- maxiMap / maxiConvert
        {
            maxiMapBank m(V);
            std::vector<double> h;
            bool ok = true;
            m.linlin(N, dx.get(), -0.5, 0.75, 100.0, 4000.0, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) {
                double v = x[i] > 0.75 ? 0.75 : x[i];
                v = v < -0.5 ? -0.5 : v;
                ok = ok && h[i] == ((v - -0.5) / (0.75 - -0.5) * (4000.0 - 100.0)) + 100.0;
            }
            EXPECT(ok);
            DeviceArray<double> ip(E);
            ip.upload(x);
            m.linlin(N, ip.get(), -0.5, 0.75, 100.0, 4000.0, ip.get());  // in place
            EXPECT(same(ip.download(), h));
            m.clamp(N, dx.get(), -0.25, 0.5, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) ok = ok && h[i] == (x[i] > 0.5 ? 0.5 : (x[i] < -0.25 ? -0.25 : x[i]));
            EXPECT(ok);
            double w_linexp = 0, w_dbs = 0, w_explin = 0, w_amp = 0;
            m.linexp(N, dx.get(), -1.0, 1.0, 20.0, 2000.0, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) {
                double v = x[i] > 1.0 ? 1.0 : x[i];
                v = v < -1.0 ? -1.0 : v;
                w_linexp = fmax(w_linexp, ulps(h[i], pow((2000.0 / 20.0), (v - -1.0) / (1.0 - -1.0)) * 20.0));
            }
            m.explin(N, dx.get(), 0.1, 1.0, 0.0, 10.0, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) {
                double v = x[i] > 1.0 ? 1.0 : x[i];
                v = v < 0.1 ? 0.1 : v;
                const double l = log(v / 0.1), den = log(1.0 / 0.1), e = (l / den * (10.0 - 0.0)) + 0.0;
                w_explin = fmax(w_explin, fabs(h[i] - e) / explin_bound(l, den, 10.0 - 0.0, e));
            }
            std::vector<double> pos(E);
            for (size_t i = 0; i < E; i++) pos[i] = fabs(x[i]) + 0.001;
            DeviceArray<double> dp(E);
            dp.upload(pos);
            m.ampToDbs(N, dp.get(), o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) w_amp = fmax(w_amp, fabs(h[i] - log10(pos[i]) * 20.0) / amptodbs_bound(log10(pos[i]) * 20.0));
            m.dbsToAmp(N, o1.get(), o2.get());  // back again, on the device
            const std::vector<double> back = o2.download();
            for (size_t i = 0; i < E; i++) w_dbs = fmax(w_dbs, ulps(back[i], pow(10.0, h[i] * 0.05)));
            printf("facade_classic_smoke: linexp within %.1f ULP, dbsToAmp within %.1f ULP, explin at %.2f and ampToDbs at %.2f of their bounds (host libm)\n",
                   w_linexp, w_dbs, w_explin, w_amp);
            // 35 and 17 ULP; explin and ampToDbs: the error of every element over its own bound
            EXPECT(w_linexp <= 35 && w_dbs <= 17 && w_explin <= 1.0 && w_amp <= 1.0);
        }
        // refused arguments say which
        EXPECT(mxg_map_render(9, V, N, dx.get(), nullptr, nullptr, o1.get(), nullptr) < 0 && strstr(mxg_last_error(), "mode"));
        EXPECT(mxg_envelope_line_render(V, N, 65, dx.get(), nullptr, nullptr, nullptr, nullptr, dx.get(), nullptr, o1.get(), nullptr) < 0 && strstr(mxg_last_error(), "S "));
        EXPECT(mxg_lag_render(V, N, dx.get(), nullptr, dx.get(), 0, dx.get(), o1.get(), nullptr) < 0 && strstr(mxg_last_error(), "d_alpha"));
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_classic_smoke: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    printf("facade_classic_smoke: ok\n");
    return 0;
}
