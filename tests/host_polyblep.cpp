// tests/host_polyblep.cpp -- host build of mxg_polyblep.h with g++ (tests/test_polyblep_host.py; pinned to
// tests/golden/polyblep.npz).  pb_host_render takes the arguments of mxg_polyblep_render (include/maxigpu.h) without the stream, on
// host arrays in the same layouts, and runs the step function the kernel of polyblep.hip runs, voice after voice.  The file has
// its own main: built as a program it plays every waveform over small shapes, the edges of every clamp of the pulse width,
// negative and zero frequencies, the fallback and phases on both sides of zero (the stand-alone run under
// -fsanitize=address,undefined); built with -shared the tests load pb_host_render.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mxg_polyblep.h"

using namespace mxg;

static const double kTab[MXG_SINTAB_LEN] = {MXG_SINTAB_VALUES};

extern "C" {

int pb_host_render(int waveform, size_t V, size_t N, const double *freq, int fps, const double *pw, double sr, double *t, double *out) {
    const PbSinTab sc = {kTab, {1.0 / 120, 1.0 / 24}};
    const bool known = pb_dispatch(waveform, [&](auto WF) {
        for (size_t v = 0; v < V; v++) {
            double tv = t[v];
            const double w = pw ? pw[v] : 0.5;
            for (size_t n = 0; n < N; n++) out[n * V + v] = pb_play<decltype(WF)::value>(tv, freq[fps ? n * V + v : v], sr, w, sc);
            t[v] = tv;
        }
    });
    return known ? 0 : -1;
}

double pb_host_sync(double phase) { return pb_sync(phase); }

}  // extern "C"

int main() {
    const double pws[] = {0.0, 0.00005, 0.0001, 0.3, 0.5, 0.9999, 0.99995, 1.0, -0.25, 1.5};
    const double frs[] = {0.0, -0.0, 1e-300, 0.125, 249.875, 250.0, 250.125, 499.0, 1000.0, 1e6, -37.5, -249.875, -251.0, -1e6, 61.7};
    const double phs[] = {2.75, -0.25, -3.0, 0.0, -0.0, 0.999999, 1.0, 123456.789, -123456.789};
    const size_t NP = sizeof(pws) / sizeof(pws[0]), NF = sizeof(frs) / sizeof(frs[0]), NH = sizeof(phs) / sizeof(phs[0]);
    double acc = 0;
    size_t count = 0;
    for (size_t V : {1, 3, 10})
        for (size_t N : {1, 7, 9, 40}) {
            std::vector<double> f(V), fb(N * V), pw(V), t(V), o(N * V);
            for (int wf = 0; wf < MXG_PBLEP_WAVEFORMS; wf++)
                for (size_t rot = 0; rot < NP; rot++) {
                    for (size_t v = 0; v < V; v++) {
                        f[v] = frs[(v + rot + wf) % NF];
                        pw[v] = pws[(v + rot) % NP];
                        t[v] = pb_host_sync(phs[(v + 2 * rot) % NH]);
                    }
                    for (size_t i = 0; i < N * V; i++) fb[i] = frs[(i * 7 + rot) % NF];
                    if (pb_host_render(wf, V, N, f.data(), 0, pw.data(), 1000.0, t.data(), o.data())) return 1;
                    if (pb_host_render(wf, V, N, fb.data(), 1, rot & 1 ? nullptr : pw.data(), 44100.0, t.data(), o.data())) return 1;
                    for (size_t i = 0; i < N * V; i++) {
                        if (o[i] == o[i] && o[i] < 1e300 && o[i] > -1e300) acc += o[i];
                        count++;
                    }
                    for (size_t v = 0; v < V; v++)
                        if (!(t[v] > -1.0 && t[v] < 1.0)) { printf("host_polyblep: phase %g left (-1, 1)\n", t[v]); return 1; }
                }
        }
    if (pb_host_render(14, 1, 1, frs, 0, nullptr, 1000.0, &acc, &acc) != -1) return 1;
    printf("host_polyblep: ok (%zu samples, %g)\n", count, acc);
    return 0;
}
