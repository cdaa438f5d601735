// tools/gen/analysis_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiZeroCrossingDetector / maxiZeroCrossingRate / maxiEnvelopeFollower / maxiSampleAndHold: tools/gen/gen_golden_analysis.py
// compiles it, together with the UNMODIFIED reference sources, into a shared library in a temporary directory and drives it
// block by block to write tests/golden/analysis.npz.
//
// V sets of objects live side by side and are called sample-major, as a patch with V analysers calls them.  The rate reads its
// window from maxiSettings::sampleRate at play time, so the harness sets that to the voice's window around the one call and
// puts the run's sample rate back for the sample-and-hold, which reads it too.  State is read through -fno-access-control, in
// the layouts of include/maxigpu.h (the ring of crossings as one byte per slot; the test packs it into bits).
#include <cstdint>
#include <vector>

#include "maximilian.h"

namespace {

struct Voice {
    maxiZeroCrossingDetector zxd;
    maxiZeroCrossingRate zcr;
    maxiEnvelopeFollower env;
    maxiSampleAndHold sah;
};
struct Bank {
    std::vector<Voice> v;
};

}  // namespace

extern "C" {

void ana_set_rate(int sr) { maxiSettings::sampleRate = sr; }

void *ana_new(size_t V) {  // the rings are sized from the sample rate in force now
    Bank *b = new Bank;
    b->v.resize(V);
    return b;
}
void ana_free(void *h) { delete (Bank *)h; }

// setAttack / setRelease per voice; coef [2][V] receives the coefficients the reference computed
void ana_set_follow(void *h, const double *attack_ms, const double *release_ms, double *coef) {
    Bank *b = (Bank *)h;
    const size_t V = b->v.size();
    for (size_t v = 0; v < V; v++) {
        b->v[v].env.setAttack(attack_ms[v]);
        b->v[v].env.setRelease(release_ms[v]);
        coef[v] = b->v[v].env.attack;
        coef[V + v] = b->v[v].env.release;
    }
}

// x [N][V]; window [V] samples; hold_ms [V] or, with hold_ps, [N][V]; outputs [N][V]
void ana_play(void *h, size_t N, const double *x, const uint32_t *window, const double *hold_ms, int hold_ps, double *zx, double *zcr,
              double *env, double *sah) {
    Bank *b = (Bank *)h;
    const size_t V = b->v.size();
    const size_t sr = maxiSettings::sampleRate;
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            Voice &o = b->v[v];
            const double s = x[n * V + v];
            zx[n * V + v] = o.zxd.zx(s) ? 1.0 : 0.0;
            maxiSettings::sampleRate = window[v];
            zcr[n * V + v] = o.zcr.play(s);
            maxiSettings::sampleRate = sr;
            env[n * V + v] = o.env.play(s);
            sah[n * V + v] = o.sah.sah(s, hold_ms[hold_ps ? n * V + v : v]);
        }
}

size_t ana_cap(void *h) { return ((Bank *)h)->v[0].zcr.buf.size(); }

// prev_x [2][V] (the detector's, the rate's own), ring u8 [cap][V], pos i32 [V], count i64 [V], dst [3][V] = env, phase, holdValue
void ana_state(void *h, double *prev_x, uint8_t *ring, int32_t *pos, int64_t *count, double *dst) {
    Bank *b = (Bank *)h;
    const size_t V = b->v.size();
    for (size_t v = 0; v < V; v++) {
        Voice &o = b->v[v];
        prev_x[v] = o.zxd.previous_x;
        prev_x[V + v] = o.zcr.zxd.previous_x;
        const size_t cap = o.zcr.buf.size();
        for (size_t s = 0; s < cap; s++) ring[s * V + v] = o.zcr.buf.buf[s] != 0.0 ? 1 : 0;
        pos[v] = (int32_t)o.zcr.buf.idx;
        count[v] = (int64_t)o.zcr.runningCount;
        dst[v] = o.env.env;
        dst[V + v] = o.sah.phase;
        dst[2 * V + v] = o.sah.holdValue;
    }
}

}  // extern "C"
