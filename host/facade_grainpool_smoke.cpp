// host/facade_grainpool_smoke.cpp -- maxiGrainPoolBank of include/maximilian_bank.hpp from plain C++ (no HIP headers): two loops are
// recorded on the device with maxiLooperBank from an oscillator bank's block, then four streams stretch them where they lie, each
// inside its own loop points (K27, mxg_granular_pool_render), in two calls.  The block, the scheduler state and the live grains are
// compared bit for bit with the library's host form (mxg_granular_pool_host) over the downloaded slots, and a checksum is printed.
// Exit status 0 = all of it held.
//
//   facade_grainpool_smoke
#include <stdio.h>
#include <string.h>

#include <vector>

#include "maximilian_bank.hpp"

using maxigpu::DeviceArray;

static int fails = 0;
#define EXPECT(c)                                                           \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "facade_grainpool_smoke: %s failed\n", #c);     \
            fails++;                                                        \
        }                                                                   \
    } while (0)

template <typename T>
static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

int main() {
    try {
        const size_t R = 2, CAP = 1500, N = 1500, S = 4, T1 = 300, T2 = 500, T = T1 + T2, RN = 40;
        maxiSettings::setup(44100, 2, 512);
        // 1. record two loops
        maxiOscBank osc(R, N);
        osc.setFrequencies({220.0, 330.0});
        DeviceArray<double> d_x(N * R, false), d_en(R);
        osc.sinewave(N, d_x.get());
        d_en.upload(std::vector<double>(R, 1.0));
        maxiLooperBank loops(R, CAP);
        loops.setLength(1, 1100);
        loops.trigger();
        loops.setRecordMix(0.0);
        loops.loopRecord(N, d_x.get(), d_en.get(), false);

        // 2. stretch them with loop points
        maxiGrainPoolBank gp(S, loops);
        gp.setSlot(2, 1);
        gp.setSlot(3, 1);
        gp.setSlot(1, 0);
        gp.setLoop(0, 0.25, 0.5);
        gp.setLoopStart(3, 0.5);
        gp.setLoopEnd(3, 0.75);
        EXPECT(gp.getLoopStart(0) == 375 && gp.getLoopEnd(0) == 750 && gp.getLoopEnd(1) == 1500 && gp.getLoopEnd(2) == 1100);
        EXPECT(gp.getLoopStart(3) == 550 && gp.getLoopEnd(3) == 825);
        const std::vector<double> pitch = {1.0, 0.5, 1.7, -1.0}, rate = {1.0, 0.25, -1.0, 2.0};
        std::vector<int32_t> rnd(S * RN);
        for (size_t s = 0; s < S; s++)
            for (size_t i = 0; i < RN; i++) rnd[s * RN + i] = (int32_t)((s * 3 + i) % 10);
        DeviceArray<double> d_pitch(S), d_rate(S), d_out(T * S, false);
        DeviceArray<int32_t> d_rnd(S * RN);
        d_pitch.upload(pitch);
        d_rate.upload(rate);
        d_rnd.upload(rnd);
        gp.stretch(T1, d_pitch.get(), false, d_rate.get(), false, 0.01, 3, nullptr, false, d_rnd.get(), RN, d_out.get());
        gp.stretch(T2, d_pitch.get(), false, d_rate.get(), false, 0.01, 3, nullptr, false, d_rnd.get(), RN, d_out.get() + T1 * S);
        maxigpu::check(mxg_sync(), "mxg_sync");
        const std::vector<double> out = d_out.download();

        // the same on the host, over what was recorded
        const size_t stride = CAP + 32;
        std::vector<double> mem(8 + R * stride, 0.0), hout(T * S), st(4 * S, 0.0), gst(32 * S, 0.0);
        for (size_t r = 0; r < R; r++) {
            const std::vector<double> a = loops.download(r);
            memcpy(mem.data() + 8 + r * stride, a.data(), a.size() * sizeof(double));
        }
        const std::vector<uint64_t> hl = {1500, 1100}, hloop = {375, 0, 0, 550, 750, 1500, 1100, 825};
        const std::vector<uint32_t> hslot = {0, 0, 1, 1};
        mxg_grain_plan *plan = mxg_grain_plan_create(0, 0.01, 44100);
        maxigpu::check(mxg_granular_pool_host(plan, 1, S, T, mem.data() + 8, stride, CAP, R, hl.data(), hslot.data(), hloop.data(), 3, pitch.data(),
                                              rate.data(), nullptr, 0, rnd.data(), RN, st.data(), gst.data(), hout.data()),
                       "mxg_granular_pool_host");
        mxg_grain_plan_destroy(plan);
        EXPECT(same(out, hout));
        EXPECT(same(gp.state(), st));
        EXPECT(same(gp.grains(), gst));
        const std::vector<double> pos = gp.getPosition();
        EXPECT(pos[0] >= 375 && pos[0] < 750 && pos[3] >= 550 && pos[3] < 825);
        double sum = 0.0, peak = 0.0;
        for (double v : out) {
            sum += v;
            peak = peak > (v < 0 ? -v : v) ? peak : (v < 0 ? -v : v);
        }
        EXPECT(peak > 0.05);

        // refused by name
        bool threw = false;
        try {
            gp.setLoop(0, 0.5, 0.5);
        } catch (const std::exception &e) {
            threw = strstr(e.what(), "loopStart >= loopEnd") != nullptr;
        }
        EXPECT(threw && gp.getLoopStart(0) == 375);
        threw = false;
        try {
            gp.setSlot(0, R);
        } catch (const std::exception &) {
            threw = true;
        }
        EXPECT(threw && gp.getSlot(0) == 0);
        printf("facade_grainpool_smoke: checksum %.17g peak %.17g\n", sum, peak);
    } catch (const std::exception &e) {
        fprintf(stderr, "facade_grainpool_smoke: %s\n", e.what());
        return 2;
    }
    if (fails) return 1;
    printf("facade_grainpool_smoke: ok\n");
    return 0;
}
