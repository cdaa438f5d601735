// tools/gen/revnet_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiReverbFilters: tools/gen/gen_golden_revnet.py compiles it, together with the UNMODIFIED reference sources, into a
// shared library in a temporary directory and calls rn_run to write the network cases of tests/golden/revnet.npz.
//
// A voice is an array of P + A maxiReverbFilters objects driven by the plain loop a patch would write:
//   acc = 0.0; acc += lowpass[c] ? comb[c].lpcombfb(x, size, fb, cut) : comb[c].combfb(x, size, fb);   c = 0 .. P-1
//   t = P ? acc : x;  t = ap[a].allpass(t, size, fb);   a = 0 .. A-1
// V voices live side by side and are called sample-major.  The state after the run is read through -fno-access-control into
// the bank layout of include/maxigpu.h: rings [V][S] with stage f (combs first) at offs[f], idx [V][P+A], lp [V][P].  Returns
// the number of ring slots beyond a stage's length that are not +0.0 (the layout relies on there being none).
//
// The objects are constructed in ZEROED memory, as the static objects of a patch are: maxiFilter's constructor leaves
// outputs[] unset, and outputs[0] is the low-pass state of lpcombfb.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "libs/maxiReverb.h"

extern "C" long rn_run(size_t V, size_t N, const double *in, int P, int A, const double *sizes, const int32_t *lowpass,
                       const double *comb_fb, const double *comb_cut, const double *ap_fb, double *out, const int32_t *offs, size_t S,
                       double *rings, int32_t *idx, double *lp) {
    maxiSettings::sampleRate = 44100;
    const int F = P + A;
    const size_t count = V * (size_t)F;
    maxiReverbFilters *obj = static_cast<maxiReverbFilters *>(std::calloc(count ? count : 1, sizeof(maxiReverbFilters)));
    for (size_t i = 0; i < count; i++) new (obj + i) maxiReverbFilters;
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            maxiReverbFilters *comb = obj + v * F, *ap = comb + P;
            const double x = in[n * V + v];
            double acc = 0.0;
            for (int c = 0; c < P; c++)
                acc += lowpass[c] ? comb[c].lpcombfb(x, sizes[c], comb_fb[v * P + c], comb_cut[v * P + c])
                                  : comb[c].combfb(x, sizes[c], comb_fb[v * P + c]);
            double t = P ? acc : x;
            for (int a = 0; a < A; a++) t = ap[a].allpass(t, sizes[P + a], ap_fb[v * A + a]);
            out[n * V + v] = t;
        }
    long stray = 0;
    for (size_t v = 0; v < V; v++)
        for (int f = 0; f < F; f++) {
            maxiReverbFilters &flt = obj[v * F + f];
            const size_t len = (size_t)sizes[f];
            for (size_t k = 0; k < len; k++) rings[v * S + offs[f] + k] = flt.delay_line[k];
            for (size_t k = len; k < flt.delay_line.size(); k++) {
                const double z = flt.delay_line[k];
                uint64_t b;
                std::memcpy(&b, &z, 8);
                if (b) stray++;
            }
            idx[v * F + f] = flt.delay_index;
            if (f < P) lp[v * P + f] = flt.mf.outputs[0];
        }
    for (size_t i = 0; i < count; i++) obj[i].~maxiReverbFilters();
    std::free(obj);
    return stray;
}
