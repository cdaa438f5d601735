// host/facade_shaper_smoke.cpp -- maxiShaperBank, maxiXFadeBank, maxiSelectBank and maxiLineBank of include/maximilian_bank.hpp
// from plain C++ (no HIP headers).  Checks what needs no reference: every bit-exact call equals the same expression written
// out here; softclip agrees with (x * x) * x to the bit and the clipped branches give exactly +-1; atanDist and asymclip stay
// within the bounds of DESIGN.md section 4 of the host libm's value; shaping in place equals shaping into a second block; a
// cross-fade of C = 2 channels applies one pair of gains to both; the selects clamp, wrap and count a NaN index; a line rendered
// in uneven blocks equals the same line rendered in one, state included, and prepare() keeps the previous lineStart.
// Exit status 0 = all of it held.
//
//   facade_shaper_smoke
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "facade_shaper_smoke: %s failed\n", #c);     \
            fails++;                                                     \
        }                                                                \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(double)));
}

static double ulps(double a, double b) {  // distance in ULPs of b
    if (a == b) return 0;
    int e;
    frexp(b, &e);
    return fabs(a - b) / ldexp(1.0, e - 53);
}

static double fastatan(double x) { return (x / (1.0 + 0.28 * (x * x))); }

int main() {
    try {
        maxiSettings::setup(1000, 2, 512);
        const size_t V = 5, N = 333, E = N * V;
        std::vector<double> x(E), y(E);
        for (size_t i = 0; i < E; i++) {
            x[i] = 1.5 * (2.0 * fmod((double)i * 0.0137, 1.0) - 1.0);
            y[i] = 1.25 * (2.0 * fmod((double)i * 0.0071 + 0.3, 1.0) - 1.0);
        }
        x[7] = 1.0; x[8] = -1.0; x[9] = 0.0; x[11] = -0.0;
        DeviceArray<double> dx(E), dy(E), o1(E), o2(2 * E);
        dx.upload(x);
        dy.upload(y);
        maxiShaperBank sh(V);
        const std::vector<double> shape = {0.5, 1.0, 3.7, 12.0, 50.0}, ea = {0.25, 0.7, 1.0, 3.0, 8.0}, eb = {8.0, 2.5, 1.0, 0.6, 0.25};
        std::vector<double> h;
        bool ok = true;
        sh.hardclip(N, dx.get(), o1.get());
        h = o1.download();
        for (size_t i = 0; i < E; i++) ok = ok && h[i] == (x[i] >= 1 ? 1 : (x[i] <= -1 ? -1 : x[i]));
        EXPECT(ok);
        sh.softclip(N, dx.get(), o1.get());
        h = o1.download();
        for (size_t i = 0; i < E; i++) {
            const double e = x[i] >= 1 ? 1 : (x[i] <= -1 ? -1 : (2 / 3.0) * (x[i] - ((x[i] * x[i]) * x[i]) / 3.0));
            ok = ok && h[i] == e && (fabs(x[i]) < 1 || fabs(h[i]) == 1);
        }
        EXPECT(ok && h[7] == 1.0 && h[8] == -1.0);
        sh.fastatan(N, dx.get(), o1.get());
        h = o1.download();
        for (size_t i = 0; i < E; i++) ok = ok && h[i] == fastatan(x[i]);
        sh.fastAtanDist(N, dx.get(), shape, o1.get());
        h = o1.download();
        for (size_t i = 0; i < E; i++) ok = ok && h[i] == (1.0 / fastatan(shape[i % V])) * fastatan(x[i] * shape[i % V]);
        EXPECT(ok);
        double worst_atan = 0, worst_pow = 0;
        sh.atanDist(N, dx.get(), shape, o1.get());
        h = o1.download();
        for (size_t i = 0; i < E; i++) worst_atan = fmax(worst_atan, ulps(h[i], (1.0 / atan(shape[i % V])) * atan(x[i] * shape[i % V])));
        sh.asymclip(N, dx.get(), ea, eb, o1.get());
        h = o1.download();
        for (size_t i = 0; i < E; i++) {
            const double a = ea[i % V], b = eb[i % V], s = x[i];
            const double e = s >= 1 ? 1 : (s <= -1 ? -1 : (s < 0 ? -(pow(-s, a)) : pow(s, b)));
            worst_pow = fmax(worst_pow, ulps(h[i], e));
            ok = ok && (fabs(s) < 1 || h[i] == e);
        }
        printf("facade_shaper_smoke: atanDist within %.1f ULP, asymclip within %.1f ULP of the host libm\n", worst_atan, worst_pow);
        EXPECT(ok && worst_atan <= 13 && worst_pow <= 17);
        // in place
        sh.fastAtanDist(N, dx.get(), 2.5, o1.get());
        DeviceArray<double> ip(E);
        ip.upload(x);
        sh.fastAtanDist(N, ip.get(), 2.5, ip.get());
        EXPECT(same(o1.download(), ip.download()));
        // a parameter per sample that repeats the per-voice value gives the per-voice bits
        {
            std::vector<double> blk(E);
            for (size_t i = 0; i < E; i++) blk[i] = shape[i % V];
            DeviceArray<double> ds(E);
            ds.upload(blk);
            sh.fastAtanDist(N, dx.get(), shape, o1.get());
            sh.fastAtanDist(N, dx.get(), ds.get(), ip.get());
            EXPECT(same(o1.download(), ip.download()));
        }
        // cross-fade: C = 2, one pair of gains for both channels
        {
            std::vector<double> c1(2 * E), c2(2 * E);
            for (size_t i = 0; i < E; i++) { c1[i] = x[i]; c1[E + i] = y[i]; c2[i] = y[i]; c2[E + i] = -x[i]; }
            DeviceArray<double> d1(2 * E), d2(2 * E);
            d1.upload(c1);
            d2.upload(c2);
            maxiXFadeBank xf(V, 2);
            xf.xfade(N, d1.get(), d2.get(), dx.get(), o2.get());  // the xfader per sample: x passes both clamps
            h = o2.download();
            for (size_t i = 0; i < E; i++) {
                double f = x[i] > 1 ? 1 : (x[i] < -1 ? -1 : x[i]);
                const double n = ((f - -1.0) / (1.0 - -1.0) * (1.0 - 0.0)) + 0.0, g1 = sqrt(1.0 - n), g2 = sqrt(n);
                ok = ok && h[i] == (c1[i] * g1) + (c2[i] * g2) && h[E + i] == (c1[E + i] * g1) + (c2[E + i] * g2);
            }
            EXPECT(ok);
            maxiXFadeBank mono(V);
            mono.xfade(N, dx.get(), dy.get(), -1.0, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) ok = ok && h[i] == x[i] + y[i] * 0.0;
            mono.xfade(N, dx.get(), dy.get(), 7.0, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) ok = ok && h[i] == x[i] * 0.0 + y[i];
            EXPECT(ok);
        }
        // selects: clamps, wrap, a NaN index
        {
            const std::vector<double> vals = {10.0, 20.0, 40.0, 80.0};
            std::vector<double> idx(E);
            for (size_t i = 0; i < E; i++) idx[i] = (x[i] + 1.5) / 3.0 * 5.0 - 0.5;  // [-0.5, 4.5]
            idx[3] = std::numeric_limits<double>::quiet_NaN();
            DeviceArray<double> di(E);
            di.upload(idx);
            maxiSelectBank s0(V, false), s1(V, true);
            s0.setValues(vals);
            s1.setValues(vals);
            s0.play(N, di.get(), false, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) {
                const double c = idx[i] < 0 ? 0 : (idx[i] >= 4 ? 3 : idx[i]);
                ok = ok && h[i] == (idx[i] != idx[i] ? vals[0] : vals[(size_t)c]);
            }
            s1.play(N, di.get(), false, o1.get());
            h = o1.download();
            bool wrapped = false;
            for (size_t i = 0; i < E; i++) {
                if (idx[i] != idx[i]) continue;
                const double c = idx[i] < 0 ? 0 : (idx[i] >= 4 ? 3 : idx[i]);
                const size_t a1 = (size_t)floor(c), a2 = a1 + 1 == 4 ? 0 : a1 + 1;
                const double mix = c - (double)a1;
                ok = ok && h[i] == (vals[a1] * (1.0 - mix)) + (vals[a2] * mix);
                wrapped = wrapped || (a1 == 3 && mix > 0);
            }
            EXPECT(ok && wrapped);
            EXPECT((s0.nanCount() == std::vector<uint32_t>{0, 0, 0, 1, 0}) && (s1.nanCount() == std::vector<uint32_t>{0, 0, 0, 1, 0}));
            // signals: K = 2 blocks, a normalised index
            std::vector<double> two(2 * E), nidx(E);
            for (size_t i = 0; i < E; i++) { two[i] = x[i]; two[E + i] = y[i]; nidx[i] = fmod((double)i * 0.013, 1.0); }
            DeviceArray<double> dt(2 * E), dn(E);
            dt.upload(two);
            dn.upload(nidx);
            s0.playSignals(N, dn.get(), 2, dt.get(), true, o1.get());
            h = o1.download();
            for (size_t i = 0; i < E; i++) ok = ok && h[i] == (nidx[i] * (2.0 - 1e-9) >= 1.0 ? y[i] : x[i]);
            EXPECT(ok);
        }
        // the line: uneven blocks against one block; prepare()'s previous lineStart; line.play(1)
        {
            std::vector<double> trig(E);
            for (size_t n = 0; n < N; n++)
                for (size_t v = 0; v < V; v++) trig[n * V + v] = (n % (40 + 7 * v)) < 10 ? 1.0 : (v & 1 ? 0.0 : -0.5);
            DeviceArray<double> dt(E);
            dt.upload(trig);
            maxiLineBank a(V), b(V);
            for (maxiLineBank *k : {&a, &b}) {
                k->prepare({0.0, 1.0, 0.25, -1.0, 0.5}, {1.0, -1.0, 0.75, 1.0, 2.0}, {20.0, 15.0, 5.0, 33.3, 0.0}, {1, 0, 0, 0, 1});
                k->triggerEnable({1.0, 1.0, 0.5, 1.0, 1.0});
            }
            a.play(N, dt.get(), o1.get());
            const size_t cuts[] = {0, 1, 8, 9, 64, 130, 131, 300, N};
            DeviceArray<double> ob(E);
            for (size_t k = 0; k + 1 < sizeof(cuts) / sizeof(cuts[0]); k++)
                b.play(cuts[k + 1] - cuts[k], dt.get() + cuts[k] * V, ob.get() + cuts[k] * V);
            h = o1.download();
            EXPECT(same(h, ob.download()));
            maxigpu::check(mxg_sync(), "mxg_sync");
            std::vector<double> sa(4 * V), sb(4 * V);
            maxigpu::check(mxg_memcpy_d2h(sa.data(), a.state(), sa.size() * sizeof(double), nullptr), "d2h");
            maxigpu::check(mxg_memcpy_d2h(sb.data(), b.state(), sb.size() * sizeof(double), nullptr), "d2h");
            EXPECT(same(sa, sb));
            const std::vector<bool> done = a.isLineComplete();
            EXPECT(done[0] && !done[1] && !done[2] && !done[3] && done[4]);
            double top = 0;
            for (size_t n = 0; n < N; n++) top = fmax(top, h[n * V]);
            EXPECT(top >= 1.0 && top < 1.06 && h[(N - 1) * V] == top);  // the one-shot line stays where it completed
            EXPECT(std::isinf(h[(N - 1) * V + 4]));                       // a duration of 0: inc = +Inf, complete on its first step
            maxiLineBank c(V);
            c.prepare(0.25, 1.0, 10.0, true);  // disabled: the line shows the previous lineStart
            c.prepare(0.75, 1.0, 10.0, true);
            c.play(7, 1.0, o1.get());
            EXPECT(o1.download()[6 * V + 2] == 0.25);
            c.triggerEnable(1.0);
            c.play(7, 1.0, o1.get());
            EXPECT(o1.download()[0] == 0.75);  // enabled and waiting (the trigger has been up all along): rewritten to lineStart
        }
        // refused arguments say which
        bool refused = false;
        try {
            maxiXFadeBank bad(V, 9);
        } catch (const std::exception &e) {
            refused = true;
        }
        EXPECT(refused);
        EXPECT(mxg_select_render(0, 65, V, N, dx.get(), dx.get(), 0, 0, nullptr, o1.get(), nullptr) < 0 && strstr(mxg_last_error(), "K "));
        EXPECT(mxg_shape_render(9, V, N, dx.get(), nullptr, nullptr, 0, o1.get(), nullptr) < 0 && strstr(mxg_last_error(), "mode"));
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_shaper_smoke: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    printf("facade_shaper_smoke: ok\n");
    return 0;
}
