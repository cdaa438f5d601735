// tools/gen/dattaro_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiDattaroReverb: tools/gen/gen_golden_dattaro.py compiles it, together with the UNMODIFIED reference sources, into a
// shared library in a temporary directory and calls dt_run to write tests/golden/dattaro.npz.
//
// V objects are constructed with maxiSettings::sampleRate = sample_rate and then played sample-major with sampleRate set
// to something else: the constructor alone fixes the lengths.  The state after the run is read through -fno-access-control
// into the bank layout of include/maxigpu.h: rings [V][S] with ring r at offs[r] in the order AP0 AP1 AP4 AP5 AP6 AP7 (=
// fArrayAllP[0, 1, 4 .. 7]) D0 .. D3 (= maxiDelays[0 .. 3]), idx [V][10], state [V][5] = fArrayLP[0 .. 2].outputs[0], sigl,
// sigr.  lens [10] and taps [14] receive the lengths and tap positions the constructor computed (fbap, dattarofixdellengths,
// dattarotapspos); fbap8 [8] the whole of fbap[0 .. 7].  Returns the number of ring slots that should be +0.0 and are not:
// beyond a ring's length, or anywhere in fArrayAllP[2] and [3], which playStereo never touches -- or -1 where offs / S do
// not fit those lengths.
//
// The objects are constructed in ZEROED memory, as the static objects of a patch are: maxiFilter's constructor leaves
// outputs[] unset, and outputs[0] is the state of the three low-passes.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "libs/maxiReverb.h"

namespace {
long nonzero(maxiReverbFilters &f, size_t from) {
    long n = 0;
    for (size_t k = from; k < f.delay_line.size(); k++) {
        const double z = f.delay_line[k];
        uint64_t b;
        std::memcpy(&b, &z, 8);
        if (b) n++;
    }
    return n;
}
}  // namespace

extern "C" long dt_run(size_t sample_rate, size_t V, size_t N, const double *in, double *out, const int32_t *offs, size_t S,
                       double *rings, int32_t *idx, double *state, int32_t *lens, int32_t *taps, int32_t *fbap8) {
    typedef maxiDattaroReverb T;
    maxiSettings::sampleRate = sample_rate;
    T *p = static_cast<T *>(std::calloc(V, sizeof(T)));
    for (size_t v = 0; v < V; v++) new (p + v) T;
    maxiSettings::sampleRate = 12345;  // a later change does nothing to an existing object
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            const double *o = p[v].playStereo(in[n * V + v]);
            out[n * V + v] = o[0];
            out[(N + n) * V + v] = o[1];
        }
    long stray = 0;
    for (int i = 0; i < 8; i++) fbap8[i] = (int32_t)p[0].fbap[i];
    for (int j = 0; j < 14; j++) taps[j] = p[0].dattarotapspos[j];
    for (int r = 0; r < 10; r++)
        lens[r] = r < 2 ? (int32_t)p[0].fbap[r] : r < 6 ? (int32_t)p[0].fbap[r + 2] : p[0].dattarofixdellengths[r - 6];
    size_t sum = 0;
    for (int r = 0; r < 10; r++) {
        if ((size_t)offs[r] != sum) stray = -1;
        sum += lens[r];
    }
    if (sum != S) stray = -1;
    for (size_t v = 0; v < V && stray >= 0; v++) {
        for (int r = 0; r < 10; r++) {
            maxiReverbFilters &f = r < 2 ? p[v].fArrayAllP[r] : r < 6 ? p[v].fArrayAllP[r + 2] : p[v].maxiDelays[r - 6];
            for (int k = 0; k < lens[r]; k++) rings[v * S + offs[r] + k] = f.delay_line[k];
            stray += nonzero(f, lens[r]);
            idx[v * 10 + r] = f.delay_index;
        }
        stray += nonzero(p[v].fArrayAllP[2], 0) + nonzero(p[v].fArrayAllP[3], 0);
        for (int k = 0; k < 3; k++) state[v * 5 + k] = p[v].fArrayLP[k].outputs[0];
        state[v * 5 + 3] = p[v].sigl;
        state[v * 5 + 4] = p[v].sigr;
    }
    maxiSettings::sampleRate = 44100;
    for (size_t v = 0; v < V; v++) p[v].~T();
    std::free(p);
    return stray;
}
