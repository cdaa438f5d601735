// host/facade_looper_smoke.cpp -- maxiLooperBank of include/maximilian_bank.hpp from plain C++ (no HIP headers): a patch that
// stays on the device.  An oscillator bank's block is recorded into 8 slots (loopRecord, with the playLoop head fused behind it),
// slot 3 is played back by the ordinary sample player (mxg_sample_render, MXG_SMP_PLAYLOOP) straight from the pool, and the pool
// is normalised.  Every step is compared bit for bit with the same step done by the library's host forms (mxg_looprec_host,
// mxg_sample_pool_normalise_host: the shared arithmetic on host arrays) over the downloaded oscillator block; the player's block is
// compared with what it reads.  Exit status 0 = all of it held.
//
//   facade_looper_smoke
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "facade_looper_smoke: %s failed\n", #c);     \
            fails++;                                                     \
        }                                                                \
    } while (0)

template <typename T>
static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

int main() {
    try {
        const size_t R = 8, CAP = 700, N = 1000;  // N: several launches; slots shorter than the call, so the overdub wraps
        const size_t lens[R] = {700, 300, 50, 441, 2, 129, 128, 699};
        maxiSettings::setup(44100, 2, 512);

        // 1. an oscillator bank's block, recorded into 8 slots
        maxiOscBank osc(R, N);
        std::vector<double> f(R);
        for (size_t r = 0; r < R; r++) f[r] = 110.0 * (double)(r + 1);
        osc.setFrequencies(f);
        DeviceArray<double> d_x(N * R, false), d_en(N * R, false), d_out(N * R, false);
        osc.sinewave(N, d_x.get());
        std::vector<double> en(N * R);
        for (size_t n = 0; n < N; n++)
            for (size_t r = 0; r < R; r++) en[n * R + r] = (r == 5 || (n / 97) % (r + 2) != 1) ? 1.0 + (double)r : 0.0;  // gates, not just 0 / 1
        d_en.upload(en);

        maxiLooperBank bank(R, CAP);
        std::vector<double> ramp(CAP);
        for (size_t i = 0; i < CAP; i++) ramp[i] = (double)((int)((i * 53) % 601) - 300);
        for (size_t r = 0; r < R; r++) bank.setSample(r, std::vector<double>(ramp.begin(), ramp.begin() + lens[r]));
        bank.trigger();
        bank.setRecordMix(0.5);
        bank.setLoop(0.1, 0.6);
        bank.setPlayLoop(0.0, 1.0);
        bank.playLoop(N, d_x.get(), d_en.get(), true, d_out.get());

        // the same on the host
        const size_t stride = mxg_sample_pool_stride(CAP);
        EXPECT(stride == bank.stride());
        std::vector<double> mem(R * stride, 0.0), x(N * R), hout(N * R), mix(R, 0.5), st(R, 0.1), ed(R, 0.6), ps(R, 0.0), pe(R, 1.0);
        std::vector<double> recpos(R, 0.0), lag(R, 0.0), pos(R, 0.0);
        std::vector<uint64_t> hl(lens, lens + R);
        std::vector<uint32_t> drop(R, 0);
        double *hpool = mem.data() + 4;
        for (size_t r = 0; r < R; r++) memcpy(hpool + r * stride, ramp.data(), lens[r] * sizeof(double));
        maxigpu::check(mxg_sync(), "mxg_sync");
        d_x.download(x.data(), N * R);
        maxigpu::check(mxg_looprec_host(R, N, hpool, stride, CAP, hl.data(), x.data(), en.data(), 1, mix.data(), st.data(), ed.data(), recpos.data(),
                                        lag.data(), MXG_SMP_PLAYLOOP, ps.data(), pe.data(), pos.data(), hout.data(), drop.data()),
                       "mxg_looprec_host");
        EXPECT(same(d_out.download(), hout));
        EXPECT(same(bank.recordPosition(), recpos));
        EXPECT(same(bank.lagValue(), lag));
        EXPECT(same(bank.position(), pos));
        EXPECT(same(bank.dropped(), drop));
        for (size_t r = 0; r < R; r++) {
            EXPECT(bank.getLength(r) == lens[r]);
            EXPECT(same(bank.download(r), std::vector<double>(hpool + r * stride, hpool + r * stride + lens[r])));
        }
        size_t changed = 0;
        for (size_t i = 0; i < lens[3]; i++) changed += hpool[3 * stride + i] != ramp[i];
        EXPECT(changed > 100);  // (the slot really holds a recording)

        // 2. slot 3 through the ordinary player, straight from the pool: 4 heads in playLoop over different parts of it
        const size_t V = 4, M = 600;
        DeviceArray<double> d_ps(V), d_pe(V), d_pp(V), d_play(M * V, false);
        const std::vector<double> vs = {0.0, 0.25, 0.5, 0.1}, ve = {1.0, 0.75, 0.9, 0.2};
        d_ps.upload(vs);
        d_pe.upload(ve);
        maxigpu::check(mxg_sample_render(MXG_SMP_PLAYLOOP, V, M, bank.deviceSamples(3), bank.getLength(3), 44100, nullptr, 0, d_ps.get(), d_pe.get(),
                                         d_pp.get(), d_play.get(), nullptr),
                       "mxg_sample_render");
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> played = d_play.download();
        const double *a3 = hpool + 3 * stride;
        bool ok = true;
        for (size_t v = 0; v < V; v++) {
            double p = 0.0;  // playLoop, C:960-967
            for (size_t n = 0; n < M; n++) {
                p += 1.0;
                const double lo = (double)lens[3] * vs[v];
                if (p < lo) p = lo;
                if ((double)(long)p >= (double)lens[3] * ve[v]) p = lo;
                ok = ok && !memcmp(&played[n * V + v], &a3[(long)p], sizeof(double));
            }
        }
        EXPECT(ok);

        // 3. normalise
        bank.normalise(200.0);
        std::vector<double> level(R, 200.0);
        maxigpu::check(mxg_sample_pool_normalise_host(R, hpool, stride, CAP, hl.data(), level.data()), "mxg_sample_pool_normalise_host");
        for (size_t r = 0; r < R; r++)
            EXPECT(same(bank.download(r), std::vector<double>(hpool + r * stride, hpool + r * stride + lens[r])));
        bool guards = true;
        for (size_t r = 0; r < R; r++)
            for (size_t i = lens[r]; i < CAP + 6; i++) guards = guards && hpool[r * stride + i] == 0.0;
        EXPECT(guards);

        // refused by name
        EXPECT(mxg_looprec_render(R, 0, bank.deviceSamples(0), stride, CAP, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  MXG_LOOPER_PLAY_NONE, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) < 0 &&
               strstr(mxg_last_error(), "N is 0"));
        bool threw = false;
        try {
            bank.setLength(2, CAP + 1);
        } catch (const std::exception &e) {
            threw = strstr(e.what(), "larger than cap") != nullptr;
        }
        EXPECT(threw && bank.getLength(2) == lens[2]);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_looper_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_looper_smoke: ok\n");
    return 0;
}
