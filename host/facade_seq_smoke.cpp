// host/facade_seq_smoke.cpp -- the sequencer banks of include/maximilian_bank.hpp from plain C++ (no HIP headers).
// Checks what needs no reference: maxiSeqBank with the pattern {3, 3, 2} on a 100 Hz clock at 1000 Hz fires on the samples
// after the boundaries 0, 3/8 and 6/8 of every cycle (worked out here in plain arithmetic); a stream rendered in uneven blocks
// equals the same stream rendered in one; playValues walks its list in order; the gate is `hold` samples long; an output that
// is not asked for leaves its stage's state alone; the signal banks (maxiTriggerBank, maxiCounterBank, maxiStepBank,
// maxiIndexBank, maxiZXToPulseBank) give what the same step written out on the host gives; 65 ratios are refused.
// Exit status 0 = all of it held.
//
//   facade_seq_smoke
#include <stdio.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "facade_seq_smoke: %s failed\n", #c);     \
            fails++;                                                  \
        }                                                             \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!(a[i] == b[i])) return false;
    return true;
}

// the bank's double state followed by its clock phases
static std::vector<double> a_state(maxiSeqBank &b, size_t V = 5) {
    std::vector<double> h(6 * V);
    maxigpu::check(mxg_sync(), "mxg_sync");
    maxigpu::check(mxg_memcpy_d2h(h.data(), b.stateDoubles(), 5 * V * sizeof(double), nullptr), "d2h");
    maxigpu::check(mxg_memcpy_d2h(h.data() + 5 * V, b.clockPhase(), V * sizeof(double), nullptr), "d2h");
    return h;
}

int main() {
    try {
        maxiSettings::setup(1000, 2, 512);
        const size_t V = 5, N = 777;
        const std::vector<std::vector<double>> times = {{3, 3, 2}, {1}}, values = {{40, 80, 170}, {7}};
        std::vector<double> freq(V, 100.0), hold(V, 4.0);
        DeviceArray<double> dfreq(V), t1(N * V), x1(N * V), g1(N * V), t2(N * V), x2(N * V), g2(N * V);
        dfreq.upload(freq);
        maxiSeqBank a(V, times, values), b(V, times, values);
        a.setPattern({0, 1, 0, 1, 0});
        b.setPattern({0, 1, 0, 1, 0});
        a.setValueList({0, 1, 0, 1, 0});
        b.setValueList({0, 1, 0, 1, 0});
        a.setHold(hold);
        b.setHold(hold);
        a.render(N, dfreq.get(), t1.get(), x1.get(), g1.get());
        const size_t cuts[] = {0, 1, 8, 9, 64, 300, 513, N};
        for (size_t k = 0; k + 1 < sizeof(cuts) / sizeof(cuts[0]); k++) {
            const size_t n0 = cuts[k], n = cuts[k + 1] - cuts[k];
            b.render(n, dfreq.get(), t2.get() + n0 * V, x2.get() + n0 * V, g2.get() + n0 * V);
        }
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> ht = t1.download(), hx = x1.download(), hg = g1.download();
        EXPECT(same(ht, t2.download()) && same(hx, x2.download()) && same(hg, g2.download()));
        EXPECT(same(a_state(a), a_state(b)));
        // voice 0, by hand: the phasor's recurrence, the boundaries 3/8, 6/8 and 0 (= 8/8)
        {
            double phase = 0.0, prev = 0.0;
            bool first = true;
            const double inc = 1. / (1000.0 / 100.0), tick = 1.0 / 1000.0, bnd[3] = {3.0 / 8.0, 6.0 / 8.0, 0.0};
            size_t count = 0, pos = 2;  // playValues: counter = len - 1 at the first call
            double gate = 0;
            for (size_t n = 0; n < N; n++) {
                const double ph = phase;
                if (phase >= 1.0) phase -= 1.0;
                phase += inc;
                if (first) { first = false; prev = ph - tick; }
                if (prev > ph) prev = -tick;
                bool tr = false;
                for (double bb : bnd) tr = tr || (prev <= bb && ph > bb);
                prev = ph;
                if (tr) { count++; pos = (pos + 1) % 3; gate = 4.0; }
                EXPECT(ht[n * V] == (tr ? 1.0 : 0.0));
                EXPECT(hx[n * V] == values[0][pos]);
                EXPECT(hg[n * V] == (gate > 0 ? 1.0 : 0.0));
                if (gate > 0) gate -= 1;
                EXPECT(hx[n * V + 1] == 7.0);
            }
            EXPECT(count > 200);
        }
        // an output that is not asked for leaves its stage's state alone
        {
            const std::vector<double> before = a_state(a);
            a.render(100, dfreq.get(), t2.get(), nullptr, nullptr);
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> after = a_state(a);
            for (size_t v = 0; v < V; v++)
                for (int row = 1; row < 5; row++) EXPECT(before[row * V + v] == after[row * V + v]);
        }
        // the signal banks against the same steps written out on the host
        {
            std::vector<double> trig(N * V), idx(N * V), rst(N * V);
            for (size_t n = 0; n < N; n++)
                for (size_t v = 0; v < V; v++) {
                    trig[n * V + v] = ((n * (v + 3)) % 17 < 2) ? 1.0 : 0.0;  // pairs of consecutive 1s: they fire once
                    idx[n * V + v] = (double)((n * 7 + v) % 130) / 100.0 - 0.15;
                    rst[n * V + v] = (double)((n + 40 * v) % 200) - 100.0;
                }
            DeviceArray<double> dt(N * V), di(N * V), dr(N * V), o(N * V), dstep(V), dhold(V);
            dt.upload(trig); di.upload(idx); dr.upload(rst);
            dstep.upload(std::vector<double>{1, 2, -1, 0.5, 6});
            dhold.upload(std::vector<double>{0, 1, 2.5, 30, 3});
            const std::vector<std::vector<double>> list = {{10, 20, 30}};
            maxiTriggerBank zx(V);
            maxiCounterBank cnt(V);
            maxiStepBank stp(V, list);
            maxiIndexBank ind(V, list);
            maxiZXToPulseBank pul(V);
            zx.onZX(N, dt.get(), o.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> hz = o.download();
            cnt.count(N, dt.get(), dr.get(), o.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> hc = o.download();
            stp.pull(N, dt.get(), dstep.get(), o.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> hs = o.download();
            ind.pull(N, dt.get(), di.get(), o.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> hi = o.download();
            pul.play(N, dt.get(), dhold.get(), o.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            const std::vector<double> hp = o.download();
            const double steps[5] = {1, 2, -1, 0.5, 6}, holds[5] = {0, 1, 2.5, 30, 3};
            for (size_t v = 0; v < V; v++) {
                double prev = 1, rprev = 1, count = 0, index = 0, value = 0, hc_ = 0;
                bool first = true, rfirst = true, sfirst = true;
                for (size_t n = 0; n < N; n++) {
                    const double in = trig[n * V + v], r = rst[n * V + v];
                    const bool fire = (prev <= 0.0 || first) && in > 0;
                    prev = in; first = false;
                    const bool rfire = (rprev <= 0.0 || rfirst) && r > 0;
                    rprev = r; rfirst = false;
                    EXPECT(hz[n * V + v] == (fire ? 1.0 : 0.0));
                    if (fire) count += 1;
                    if (rfire) count = 0;
                    EXPECT(hc[n * V + v] == count);
                    if (fire) {
                        if (sfirst) { sfirst = false; index = 0; }
                        else {
                            double s = steps[v] > 3.0 ? 3.0 : steps[v];
                            index += s;
                            if (index < 0) index = 3.0 + index;
                            else if (index >= 3.0) index -= 3.0;
                        }
                        double x = idx[n * V + v];
                        x = x < 0 ? 0 : (x > 1 ? 1 : x);
                        value = list[0][(size_t)(x * 0.99999999 * 3.0)];
                        hc_ = holds[v];
                    }
                    EXPECT(hs[n * V + v] == list[0][(size_t)index]);
                    EXPECT(hi[n * V + v] == value);
                    EXPECT(hp[n * V + v] == (hc_ > 0 ? 1.0 : 0.0));
                    if (hc_ > 0) hc_ -= 1;
                }
            }
        }
        bool threw = false;
        try {
            maxiSeqBank bad(1, {std::vector<double>(65, 1.0)});
        } catch (const std::exception &) {
            threw = true;
        }
        EXPECT(threw);
        maxiSettings::setup(44100, 2, 1024);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_seq_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_seq_smoke OK\n");
    return 0;
}
