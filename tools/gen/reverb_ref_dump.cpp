// tools/gen/reverb_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiSatReverb / maxiFreeVerb / maxiFreeVerbStereo: tools/gen/gen_golden_reverb.py compiles it, together with the
// UNMODIFIED reference sources, into a shared library in a temporary directory and calls rv_run to write
// tests/golden/reverb.npz.
//
// V objects live side by side and are called sample-major, as a patch with V reverbs calls them.  mode [N] chooses, per
// sample, maxiFreeVerb's overload (0 = play(x), 1 = play(x, roomsize, absorbtion)); room / absorb are [N][V].  The state
// after the run is read through -fno-access-control into the bank layout of include/maxigpu.h: rings [V][S] with filter f
// (combs first, then allpasses) at offs[f], idx [V][F], lp [V][8], wc [V][2].  Returns the number of ring slots beyond a
// filter's length that are not +0.0 (the layout relies on there being none), or -1 for an unknown kind.
//
// The objects are constructed in ZEROED memory, as the static objects of a patch are: maxiFilter's constructor leaves
// outputs[] unset, and outputs[0] is the low-pass state of maxiFreeVerb's combs.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "libs/maxiReverb.h"

namespace {
template <class T>
struct Objects {
    T *p;
    size_t n;
    explicit Objects(size_t V) : p(static_cast<T *>(std::calloc(V, sizeof(T)))), n(V) {
        for (size_t v = 0; v < V; v++) new (p + v) T;
    }
    ~Objects() {
        for (size_t v = 0; v < n; v++) p[v].~T();
        std::free(p);
    }
    T &operator[](size_t v) { return p[v]; }
};

template <class T>
long dump(Objects<T> &obj, size_t V, int nc, int na, const int32_t *lens, const int32_t *offs, size_t S, double *rings,
          int32_t *idx, double *lp, double *wc) {
    long stray = 0;
    const int F = nc + na;
    for (size_t v = 0; v < V; v++) {
        for (int f = 0; f < F; f++) {
            maxiReverbFilters &flt = f < nc ? obj[v].fArrayTwo[f] : obj[v].fArrayAllP[f - nc];
            for (int k = 0; k < lens[f]; k++) rings[v * S + offs[f] + k] = flt.delay_line[k];
            for (size_t k = lens[f]; k < flt.delay_line.size(); k++) {
                const double z = flt.delay_line[k];
                uint64_t b;
                std::memcpy(&b, &z, 8);
                if (b) stray++;
            }
            idx[v * F + f] = flt.delay_index;
        }
        for (int c = 0; c < 8; c++) lp[v * 8 + c] = obj[v].fArrayTwo[c].mf.outputs[0];
        wc[v * 2] = obj[v].combgainweight[0];
        wc[v * 2 + 1] = obj[v].lpcombcutoff[0];
    }
    return stray;
}
}  // namespace

extern "C" long rv_run(int kind, size_t V, size_t N, const double *in, const int32_t *mode, const double *room,
                       const double *absorb, double *out, int nc, int na, const int32_t *lens, const int32_t *offs, size_t S,
                       double *rings, int32_t *idx, double *lp, double *wc) {
    maxiSettings::sampleRate = 44100;
    if (kind == 0) {
        Objects<maxiSatReverb> r(V);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) out[n * V + v] = r[v].play(in[n * V + v]);
        return dump(r, V, nc, na, lens, offs, S, rings, idx, lp, wc);
    }
    if (kind == 1) {
        Objects<maxiFreeVerb> r(V);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) {
                const size_t e = n * V + v;
                out[e] = mode[n] ? r[v].play(in[e], room[e], absorb[e]) : r[v].play(in[e]);
            }
        return dump(r, V, nc, na, lens, offs, S, rings, idx, lp, wc);
    }
    if (kind == 2) {
        Objects<maxiFreeVerbStereo> r(V);
        for (size_t n = 0; n < N; n++)
            for (size_t v = 0; v < V; v++) {
                const size_t e = n * V + v;
                const double *o = r[v].playStereo(in[e], room[e], absorb[e]);
                out[e] = o[0];
                out[N * V + e] = o[1];
            }
        return dump(r, V, nc, na, lens, offs, S, rings, idx, lp, wc);
    }
    return -1;
}
