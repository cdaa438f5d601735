// tools/gen/kuramoto_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiKuramotoOscillatorSet / maxiAsyncKuramotoOscillator: tools/gen/gen_golden_kuramoto.py compiles it, together with the
// UNMODIFIED reference sources, into a shared library in a temporary directory and drives it block by block to write
// tests/golden/kuramoto.npz.  State is read (and the async set's phases set without raising its flag) through
// -fno-access-control, in the layouts of include/maxigpu.h.
//
// The file also holds a LONG DOUBLE restatement of the same recurrence (kld_*): the same steps in the same order on 64-bit
// significands, with the reference's double constants (TWOPI, dt) taken as given.  The reference's distance from it is the size
// of the reference's own accumulated rounding: the generator stores it per case as the tolerance of that case.
#include <cmath>
#include <cstdint>
#include <vector>

#include "maximilian.h"

namespace {

struct Set {
    bool async;
    maxiKuramotoOscillatorSet *sync_set;
    maxiAsyncKuramotoOscillator *async_set;
    maxiKuramotoOscillatorSet *base() { return async ? async_set : sync_set; }
};

struct LdSet {
    bool async;
    int update;
    long double dt;
    std::vector<long double> phase, gathered;
};

}  // namespace

extern "C" {

void kura_set_rate(int sr) { maxiSettings::sampleRate = sr; }

void *kura_new(size_t N, int async) {  // dt is taken from the sample rate in force now
    Set *s = new Set{async != 0, nullptr, nullptr};
    if (async) s->async_set = new maxiAsyncKuramotoOscillator(N);
    else s->sync_set = new maxiKuramotoOscillatorSet(N);
    return s;
}
void kura_free(void *h) {
    Set *s = (Set *)h;
    delete s->sync_set;
    delete s->async_set;
    delete s;
}

// raise = 0: the phases are written without the async set's flag (fresh objects that were never told anything)
void kura_set_phases(void *h, const double *p, int raise) {
    Set *s = (Set *)h;
    const size_t N = s->base()->size();
    if (s->async && raise) {
        s->async_set->setPhases(std::vector<double>(p, p + N));
    } else {
        for (size_t i = 0; i < N; i++) s->base()->oscs[i].setPhase(p[i]);
    }
}
void kura_set_phase(void *h, double p, size_t idx) {
    Set *s = (Set *)h;
    if (s->async) s->async_set->setPhase(p, idx);
    else s->sync_set->setPhase(p, idx);
}

// freq, K: one value, or with the _ps flag one per sample; mix [B]; phases_out [B][N] = getPhase(i) after each sample
void kura_play(void *h, size_t B, const double *freq, int freq_ps, const double *K, int K_ps, double *mix, double *phases_out) {
    Set *s = (Set *)h;
    const size_t N = s->base()->size();
    for (size_t b = 0; b < B; b++) {
        const double f = freq[freq_ps ? b : 0], k = K[K_ps ? b : 0];
        mix[b] = s->async ? s->async_set->play(f, k) : s->sync_set->play(f, k);
        for (size_t i = 0; i < N; i++) phases_out[b * N + i] = s->async ? s->async_set->getPhase(i) : s->sync_set->getPhase(i);
    }
}

// phase [N], gathered [N], *update
void kura_state(void *h, double *phase, double *gathered, int32_t *update) {
    Set *s = (Set *)h;
    const size_t N = s->base()->size();
    for (size_t i = 0; i < N; i++) {
        phase[i] = s->base()->oscs[i].phase;
        gathered[i] = s->base()->phases[i];
    }
    *update = s->async ? (s->async_set->update ? 1 : 0) : 0;
}
double kura_dt(void *h) { return ((Set *)h)->base()->oscs[0].dt; }

// ---- the long double restatement --------------------------------------------------------------------------------------
void *kld_new(size_t N, int async, double dt) {
    LdSet *s = new LdSet{async != 0, 0, (long double)dt, std::vector<long double>(N, 0.0L), std::vector<long double>(N, 0.0L)};
    return s;
}
void kld_free(void *h) { delete (LdSet *)h; }
void kld_set_phases(void *h, const double *p, int raise) {
    LdSet *s = (LdSet *)h;
    for (size_t i = 0; i < s->phase.size(); i++) s->phase[i] = (long double)p[i];
    if (s->async && raise) s->update = 1;
}
void kld_set_phase(void *h, double p, size_t idx) {
    LdSet *s = (LdSet *)h;
    s->phase[idx] = (long double)p;
    if (s->async) s->update = 1;
}
void kld_play(void *h, size_t B, const double *freq, int freq_ps, const double *K, int K_ps, double *mix, double *phases_out) {
    LdSet *s = (LdSet *)h;
    const size_t N = s->phase.size();
    const long double twopi = (long double)(double)TWOPI;
    for (size_t b = 0; b < B; b++) {
        const long double f = (long double)freq[freq_ps ? b : 0];
        long double k = (long double)K[K_ps ? b : 0];
        if (!s->async || s->update) s->gathered = s->phase;
        if (s->async && !s->update) k = 0.0L;
        long double sum = 0.0L;
        for (size_t i = 0; i < N; i++) {
            long double adj = 0.0L;
            for (size_t j = 0; j < N; j++) adj += sinl(s->gathered[j] - s->phase[i]);
            long double p = s->phase[i] + s->dt * (f + ((k / (long double)N) * adj));
            if (p >= twopi) p -= twopi;
            else if (p < 0.0L) p += twopi;
            s->phase[i] = p;
            sum += p;
            phases_out[b * N + i] = (double)p;
        }
        s->update = 0;
        mix[b] = (double)(sum / (long double)N);
    }
}

}  // extern "C"
