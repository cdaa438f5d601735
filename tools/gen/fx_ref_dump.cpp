// tools/gen/fx_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiFlanger / maxiChorus: tools/gen/gen_golden_fx.py compiles it, together with the UNMODIFIED reference sources,
// into a shared library in a temporary directory and calls these two functions to write tests/golden/fx.npz.
//
// V objects live side by side and are called sample-major (sample n of every voice, then sample n+1), as a patch
// with V effects calls them.  Each object is reset by value-initialisation (`new (p) maxiFlanger()`), which zeroes
// maxiDelayline::phase -- a member no constructor sets (H:269) -- as static objects have it.
// Parameters are [N][V] arrays (a block-rate parameter is the same value in every row).  The state after the run
// is read back through -fno-access-control.
#include <cstdint>
#include <cstdlib>
#include <new>
#include <vector>

#include "maximilian.h"

template <class T>
static std::vector<T *> make_objects(size_t V) {
    std::vector<T *> objs(V);
    for (size_t v = 0; v < V; v++) objs[v] = new (std::malloc(sizeof(T))) T();  // value-initialised
    return objs;
}
template <class T>
static void free_objects(std::vector<T *> &objs) {
    for (T *o : objs) {
        o->~T();
        std::free(o);
    }
}

extern "C" {

// out [N][V]; state: dl_phase [V], lfo_phase [V]
int fx_flange(size_t V, size_t N, const double *in, const uint32_t *delay, const double *feedback, const double *speed,
              const double *depth, double *out, int32_t *dl_phase, double *lfo_phase) {
    maxiSettings::sampleRate = 44100;
    std::vector<maxiFlanger *> f = make_objects<maxiFlanger>(V);
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            const size_t e = n * V + v;
            out[e] = f[v]->flange(in[e], delay[e], feedback[e], speed[e], depth[e]);
        }
    for (size_t v = 0; v < V; v++) {
        dl_phase[v] = f[v]->dl.phase;
        lfo_phase[v] = f[v]->lfo.phase;
    }
    free_objects(f);
    return 0;
}

// The draws: srand(seed), record N*V rand() in call order; srand(seed) again, run.  rand_out [N][V], out [N][V];
// state: dl_phase [2][V], lp [2][V] (lopass x, y)
int fx_chorus(size_t V, size_t N, const double *in, const uint32_t *delay, const double *feedback, const double *speed,
              const double *depth, unsigned seed, int32_t *rand_out, double *out, int32_t *dl_phase, double *lp) {
    maxiSettings::sampleRate = 44100;
    std::srand(seed);
    for (size_t e = 0; e < N * V; e++) rand_out[e] = std::rand();
    std::srand(seed);
    std::vector<maxiChorus *> c = make_objects<maxiChorus>(V);
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            const size_t e = n * V + v;
            out[e] = c[v]->chorus(in[e], delay[e], feedback[e], speed[e], depth[e]);
        }
    for (size_t v = 0; v < V; v++) {
        dl_phase[v] = c[v]->dl.phase;
        dl_phase[V + v] = c[v]->dl2.phase;
        lp[v] = c[v]->lopass.x;
        lp[V + v] = c[v]->lopass.y;
    }
    free_objects(c);
    return 0;
}

}  // extern "C"
