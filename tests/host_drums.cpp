// tests/host_drums.cpp -- host build of mxg_drums.h with g++ (tests/test_drums_host.py; pinned to tests/golden/drums.npz).
// dr_host_render / dr_host_clock take the arguments of mxg_drum_render / mxg_clock_render (include/maxigpu.h) without the stream, plus
// the sample rate, on host arrays in the same layouts, and run the step functions the kernels of drums.hip run, voice after voice.
// The file has its own main: built as a program it plays every drum with every combination of the four switches over small shapes,
// shared and per-voice triggers, no trigger block, zero and huge pitches and denormal envelope amplitudes (the stand-alone run
// under -fsanitize=address,undefined); built with -shared the tests load the two functions.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mxg_drums.h"
#include "maxi_tables.h"

using namespace mxg;

static const double kSinTab[MXG_SINTAB_LEN] = {MXG_SINTAB_VALUES};
static const double kSineBuf[MAXI_SINE_TAB_LEN] = MAXI_SINE_TAB_INIT;

extern "C" {

int dr_host_render(int kind, int flags, size_t V, size_t N, const double *trig, int tpv, const int32_t *rnd, const double *pitch,
                   const double *env_par, const int64_t *holdtime, const double *shape, const double *coef, const double *gain,
                   double sr, double *phase, double *dst, int64_t *ist, double *fst, double *out) {
    const DrumArgs A = {V, N, tpv ? V : 1, pitch, env_par, holdtime, shape, coef, gain, sr, flags, phase, dst, ist, fst, 0};
    return drum_dispatch(kind, [&](auto K) { drum_host_run<decltype(K)::value>(A, trig, tpv, rnd, out, kSinTab, kSineBuf); }) ? 0 : -1;
}

int dr_host_clock(size_t V, size_t N, const double *bps, double sr, double *clk, const int32_t *lastcount, int64_t *playhead,
                  int32_t *count, double *tick) {
    for (size_t v = 0; v < V; v++) {
        const OscPre q = osc_pre<MXG_OSC_PHASOR>(bps[v], sr, 0.0, 0.0);
        long long ph = playhead[v];
        int32_t cur = 0;
        for (size_t n = 0; n < N; n++) tick[n * V + v] = clock_tick(clk[v], q, lastcount ? lastcount[v] : 0, cur, ph) ? 1.0 : 0.0;
        playhead[v] = ph;
        count[v] = cur;
    }
    return 0;
}

}  // extern "C"

int main() {
    const double pitches[] = {0.0, 200.0, 800.0, 12000.0, 1e9, -50.0, 1e-300};
    const double hat_pitches[] = {0.0, 200.0, 800.0, 12000.0, 20000.0, 50.0, 1e-300};  // sinebuf's domain: 0 <= pitch < sampleRate
    const size_t NP = sizeof(pitches) / sizeof(pitches[0]);
    double acc = 0;
    size_t count = 0;
    uint32_t lcg = 12345;
    for (size_t V : {1, 3, 10})
        for (size_t N : {1, 7, 9, 40}) {
            std::vector<double> trig(N * V), pitch(V), par(4 * V), shape(V), coef(5 * V), gain(V), phase(V), dst(2 * V), fst(3 * V), out(N * V), tick(N * V);
            std::vector<int64_t> hold(V), ist(6 * V), playhead(V);
            std::vector<int32_t> rnd(N * V), last(V), cnt(V);
            for (int kind = 0; kind < MXG_DRUM_KINDS; kind++)
                for (int flags = 0; flags < 16; flags++)
                    for (int tpv = 0; tpv < 3; tpv++) {
                        for (size_t v = 0; v < V; v++) {
                            pitch[v] = (kind == MXG_DRUM_HATS ? hat_pitches : pitches)[(v + flags + kind) % NP];
                            par[v] = (v & 1) ? 1.0 : 0.25;
                            par[V + v] = 0.9;
                            par[2 * V + v] = 0.3;
                            par[3 * V + v] = (v % 3) ? 0.97 : 0.3;
                            hold[v] = 1 + (v % 3);
                            shape[v] = 0.5 + v;
                            gain[v] = 0.5 + 0.75 * v;
                            for (int r = 0; r < 5; r++) coef[r * V + v] = 0.05 + 0.1 * r;
                            phase[v] = 0.0;
                            dst[v] = (v == 2) ? 3 * 4.9406564584124654e-324 : 0.0;  // a denormal amplitude in release
                            dst[V + v] = 0.0;
                            for (int r = 0; r < 6; r++) ist[r * V + v] = 0;
                            if (v == 2) { ist[v] = hold[v]; ist[5 * V + v] = 1; }
                            for (int r = 0; r < 3; r++) fst[r * V + v] = 0.0;
                        }
                        for (size_t i = 0; i < N * V; i++) {
                            lcg = lcg * 1664525u + 1013904223u;
                            rnd[i] = (int32_t)(lcg >> 1);
                            trig[i] = (lcg >> 28) == 0 || i == 0 ? 1.0 : 0.0;
                        }
                        if (dr_host_render(kind, flags, V, N, tpv == 2 ? nullptr : trig.data(), tpv == 1, kind ? rnd.data() : nullptr, pitch.data(),
                                           par.data(), hold.data(), shape.data(), coef.data(), gain.data(), flags & 1 ? 48000.0 : 44100.0,
                                           phase.data(), dst.data(), ist.data(), fst.data(), out.data()))
                            return 1;
                        for (size_t i = 0; i < N * V; i++) {
                            if (out[i] == out[i] && out[i] < 1e300 && out[i] > -1e300) acc += out[i];
                            count++;
                        }
                    }
            for (size_t v = 0; v < V; v++) { pitch[v] = 600.0 + 100.0 * v; phase[v] = 0.0; playhead[v] = 0; last[v] = (int32_t)(v & 1); }
            if (dr_host_clock(V, N, pitch.data(), 44100.0, phase.data(), last.data(), playhead.data(), cnt.data(), tick.data())) return 1;
            for (size_t i = 0; i < N * V; i++) acc += tick[i];
        }
    if (dr_host_render(3, 0, 1, 1, nullptr, 0, nullptr, &acc, &acc, nullptr, nullptr, nullptr, nullptr, 44100.0, &acc, &acc, nullptr, &acc, &acc) != -1) return 1;
    printf("host_drums: ok (%zu samples, %g)\n", count, acc);
    return 0;
}
