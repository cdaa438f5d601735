// host/facade_drums_smoke.cpp -- maxiKickBank / maxiSnareBank / maxiHatsBank / maxiClockBank of include/maximilian_bank.hpp from
// plain C++ (no HIP headers).  Checks what needs no reference: a clock bank's tick block drives the three drum banks device to
// device, rendered in uneven blocks with a setter between two blocks, and equals mxg_clock_host + mxg_drum_host (the same arithmetic
// on the CPU) called on the same blocks with the same parameters -- bit for bit for the ticks, snare, hats and every state array,
// within 2^-52 for the kick (one sine of <= 1 ULP times envOut <= 1, one rounding; its switches are off here); a fresh bank is
// silent until it is triggered; a wrong vector length is refused.
// Exit status 0 = all of it held.
//
//   facade_drums_smoke
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                       \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "facade_drums_smoke: %s failed\n", #c);     \
            fails++;                                                    \
        }                                                               \
    } while (0)

template <typename T>
static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

// the host mirror of one drum bank: mxg_drum_host on the same parameters
struct HostDrum {
    int kind, flags;
    size_t V;
    std::vector<double> pitch, env, shape, coef, gain, phase, dst, fst;
    std::vector<int64_t> hold, ist;
    HostDrum(int k, int f, size_t v, double pitch_, double decay, double sustain, double release, double dist, double g)
        : kind(k), flags(f), V(v), pitch(v, pitch_), env(4 * v), shape(v, dist), coef(5 * v), gain(v, g), phase(v), dst(2 * v), fst(3 * v),
          hold(v, 1), ist(6 * v) {
        const double e[4] = {mxg_env_coeff_host(0, 0), mxg_env_coeff_host(1, decay), sustain, mxg_env_coeff_host(2, release)};
        for (int r = 0; r < 4; r++) std::fill(env.begin() + r * V, env.begin() + (r + 1) * V, e[r]);
    }
    void release(double ms) { std::fill(env.begin() + 3 * V, env.end(), mxg_env_coeff_host(2, ms)); }
    void render(size_t N, const double *trig, const int32_t *rnd, double *out) {
        maxigpu::check(mxg_drum_host(kind, flags, V, N, trig, 1, rnd, pitch.data(), env.data(), hold.data(), shape.data(), coef.data(),
                                     gain.data(), phase.data(), dst.data(), ist.data(), fst.data(), out), "mxg_drum_host");
    }
};

int main() {
    try {
        maxiSettings::setup(48000, 2, 512);
        const size_t V = 67, N = 700, E = N * V;
        const size_t cuts[] = {0, 1, 9, 144, 145, 657, N};
        maxiClockBank clock(V);
        clock.setTicksPerBeat(4);
        clock.setTempo(9000);  // bps 600
        maxiKickBank kick(V);
        maxiSnareBank snare(V);
        maxiHatsBank hats(V);
        kick.setRelease(4);
        snare.setRelease(6), snare.setDecay(3), snare.setCutoff(3000), snare.setResonance(3), snare.setDistortion(3), snare.setGain(1.7);
        snare.useDistortion = snare.useLimiter = snare.inverse = true;
        hats.setRelease(3), hats.setDecay(2), hats.setFilterCutoff(7000), hats.setFilterResonance(2), hats.setGain(2);
        hats.useFilter = hats.useLimiter = true;
        HostDrum hk(MXG_DRUM_KICK, 0, V, 200, 1, 1, 4, 0, 1);
        HostDrum hs(MXG_DRUM_SNARE, 15, V, 800, 3, 0.05, 6, 3, 1.7);
        HostDrum hh(MXG_DRUM_HATS, MXG_DRUM_FILTER | MXG_DRUM_LIMITER, V, 12000, 2, 0.1, 3, 0, 2);
        {
            std::vector<double> cu(V, 3000.), re(V, 3.), c3(3 * V);
            maxigpu::check(mxg_filter_coeffs_host(MXG_FLT_LORES, V, cu.data(), re.data(), c3.data()), "mxg_filter_coeffs_host");
            std::copy(c3.begin(), c3.end(), hs.coef.begin());
            std::fill(cu.begin(), cu.end(), 7000.), std::fill(re.begin(), re.end(), 2.);
            maxigpu::check(mxg_svf_coeffs_host(V, cu.data(), re.data(), hh.coef.data()), "mxg_svf_coeffs_host");
        }
        std::vector<int32_t> draws(E);
        uint32_t lcg = 1;
        for (auto &d : draws) { lcg = lcg * 1664525u + 1013904223u; d = (int32_t)(lcg >> 1); }
        DeviceArray<int32_t> d_draws(E);
        d_draws.upload(draws);
        DeviceArray<double> d_tick(E), ok(E), os(E), oh(E);
        std::vector<double> bps(V, 600.), clk(V, 0.), tick(E), ek(E), es(E), eh(E);
        std::vector<int64_t> ph(V, 0);
        std::vector<int32_t> cnt(V);
        for (size_t b = 0; b + 1 < sizeof(cuts) / sizeof(cuts[0]); b++) {
            const size_t a = cuts[b], n = cuts[b + 1] - a;
            if (a == 145) {  // a setter between two blocks
                snare.setRelease(9);
                hs.release(9);
            }
            clock.render(n, d_tick.get() + a * V);
            kick.render(n, d_tick.get() + a * V, true, nullptr, ok.get() + a * V);
            snare.render(n, d_tick.get() + a * V, true, d_draws.get() + a * V, os.get() + a * V);
            hats.render(n, d_tick.get() + a * V, true, d_draws.get() + a * V, oh.get() + a * V);
            maxigpu::check(mxg_clock_host(V, n, bps.data(), clk.data(), nullptr, ph.data(), cnt.data(), tick.data() + a * V), "mxg_clock_host");
            hk.render(n, tick.data() + a * V, nullptr, ek.data() + a * V);
            hs.render(n, tick.data() + a * V, draws.data() + a * V, es.data() + a * V);
            hh.render(n, tick.data() + a * V, draws.data() + a * V, eh.data() + a * V);
        }
        maxigpu::check(mxg_sync(), "mxg_sync");
        EXPECT(same(d_tick.download(), tick));
        EXPECT(same(clock.playHead(), ph) && ph[0] > 5);
        EXPECT(same(clock.currentCount(), cnt));
        EXPECT(same(clock.phase().download(), clk));
        EXPECT(same(os.download(), es));
        EXPECT(same(oh.download(), eh));
        EXPECT(same(snare.phase().download(), hs.phase) && same(snare.dstate().download(), hs.dst) && same(snare.istate().download(), hs.ist) &&
               same(snare.fstate().download(), hs.fst));
        EXPECT(same(hats.phase().download(), hh.phase) && same(hats.dstate().download(), hh.dst) && same(hats.istate().download(), hh.ist) &&
               same(hats.fstate().download(), hh.fst));
        EXPECT(same(kick.phase().download(), hk.phase) && same(kick.dstate().download(), hk.dst) && same(kick.istate().download(), hk.ist));
        const std::vector<double> gk = ok.download(), gs = os.download();
        double worst = 0, peak = 0, clipped = 0;
        for (size_t i = 0; i < E; i++) {
            worst = fmax(worst, fabs(gk[i] - ek[i]));
            peak = fmax(peak, fabs(gk[i]));
            clipped += fabs(gs[i]) == 1.0;
        }
        EXPECT(worst <= ldexp(1.0, -52) && peak > 0.5);
        EXPECT(clipped > 30);
        {  // never triggered: silence
            maxiHatsBank quiet(V);
            quiet.render(64, nullptr, false, d_draws.get(), oh.get());
            maxigpu::check(mxg_sync(), "mxg_sync");
            std::vector<double> q(64 * V);
            oh.download(q.data(), q.size());
            bool zero = true;
            for (double x : q) zero = zero && x == 0.0;
            EXPECT(zero);
        }
        bool refused = false;
        try {
            kick.setPitch(std::vector<double>(V + 1, 100.));
        } catch (const std::exception &) {
            refused = true;
        }
        EXPECT(refused);
        printf("facade_drums_smoke: %s (kick within %.3g of the host arithmetic)\n", fails ? "FAILED" : "ok", worst);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_drums_smoke: %s\n", e.what());
        return 2;
    }
    return fails ? 1 : 0;
}
