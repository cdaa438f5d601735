// tools/gen/dyn_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiDynamics / maxiRMS: tools/gen/gen_golden_dyn.py compiles it, together with the UNMODIFIED reference sources, into
// a shared library in a temporary directory and drives it block by block to write tests/golden/dyn.npz.
//
// V objects live side by side and are called sample-major, as a patch with V compressors calls them.  They are built
// in zeroed memory (calloc + placement new): maxiEnvGen::nxcHappened has no initialiser and is only assigned when the
// envelope is triggered, static objects have it false.  The rings are sized in the constructor from the sample rate in
// force at that moment (sr_ctor), every later conversion uses sr_run.  The constructors' "Stage ..." lines go to the
// caller's stdout.  State is read through -fno-access-control, in the layouts of include/maxigpu.h.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <vector>

#include "maximilian.h"

namespace {

struct Bank {
    std::vector<maxiDynamics *> d;
    std::vector<int> analyser;
};

struct RmsBank {
    std::vector<maxiRMS *> r;
};

void dump_env(maxiEnvGen &e, size_t V, size_t v, double *dst, int64_t *ist, double *stages) {
    const bool in = e.phase < e.stages.size();
    dst[v] = e.envval;
    dst[V + v] = in ? e.stages[e.phase].currentlevel : 0.0;
    dst[2 * V + v] = e.trigDetector.previousValue;
    dst[3 * V + v] = e.holdDetector.previousValue;
    dst[4 * V + v] = e.retriggerDetector.previousValue;
    ist[v] = (int64_t)e.phase;
    ist[V + v] = (int64_t)e.state;
    ist[2 * V + v] = e.nxcHappened;
    ist[3 * V + v] = in ? (int64_t)e.stages[e.phase].counter : 0;
    ist[4 * V + v] = e.trigDetector.firstTrigger;
    ist[5 * V + v] = e.holdDetector.firstTrigger;
    ist[6 * V + v] = e.retriggerDetector.firstTrigger;
    if (stages)
        for (size_t i = 0; i < e.stages.size(); i++) {
            double *st = stages + 6 * i;
            st[0] = e.stages[i].startlevel; st[1] = e.stages[i].endlevel; st[2] = e.stages[i].gradient;
            st[3] = e.stages[i].curve; st[4] = (double)e.stages[i].length; st[5] = e.stages[i].hold;
        }
}

}  // namespace

extern "C" {

void *dyn_new(size_t V, int sr_ctor, int sr_run) {
    Bank *b = new Bank;
    maxiSettings::sampleRate = sr_ctor;
    for (size_t v = 0; v < V; v++) b->d.push_back(new (std::calloc(1, sizeof(maxiDynamics))) maxiDynamics());
    b->analyser.assign(V, 1);
    maxiSettings::sampleRate = sr_run;
    return b;
}

void dyn_free(void *h) {
    Bank *b = (Bank *)h;
    for (maxiDynamics *o : b->d) {
        o->~maxiDynamics();
        std::free(o);
    }
    delete b;
}

// what: 0 setAttackHigh 1 setReleaseHigh 2 setAttackLow 3 setReleaseLow 4 setLookAhead 5 setRMSWindowSize 6 setInputAnalyser
int dyn_set(void *h, int what, size_t v, double value) {
    Bank *b = (Bank *)h;
    maxiDynamics &d = *b->d[v];
    switch (what) {
        case 0: d.setAttackHigh(value); break;
        case 1: d.setReleaseHigh(value); break;
        case 2: d.setAttackLow(value); break;
        case 3: d.setReleaseLow(value); break;
        case 4: d.setLookAhead(value); break;
        case 5: d.setRMSWindowSize(value); break;
        case 6:
            d.setInputAnalyser(value != 0 ? maxiDynamics::RMS : maxiDynamics::PEAK);
            b->analyser[v] = value != 0;
            break;
        default: return -1;
    }
    return 0;
}

// par: six [N][V] arrays (thresholdHigh, ratioHigh, kneeHigh, thresholdLow, ratioLow, kneeLow).  level_db [N][V]: the detector
// level in dB the call just compared, recomputed from the object's state after the call (RMS: sqrt(runningRMS / windowSize),
// the expression maxiRMS::play returned; PEAK: the double abs).
int dyn_play(void *h, size_t N, const double *sig, const double *control, const double *const *par, double *out,
             double *level_db) {
    Bank *b = (Bank *)h;
    const size_t V = b->d.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            const size_t e = n * V + v;
            maxiDynamics &d = *b->d[v];
            out[e] = d.play(sig[e], control[e], par[0][e], par[1][e], par[2][e], par[3][e], par[4][e], par[5][e]);
            const double level = b->analyser[v] ? std::sqrt(d.rms.runningRMS / d.rms.windowSize) : std::fabs(control[e]);
            level_db[e] = std::log10(level) * 20.0;
        }
    return 0;
}

void dyn_sizes(void *h, int64_t *cap_rms, int64_t *cap_la) {
    Bank *b = (Bank *)h;
    *cap_rms = (int64_t)b->d[0]->rms.buf.size();
    *cap_la = (int64_t)b->d[0]->lookAheadDelay.size();
}

// rring [cap_rms][V], lring [cap_la][V], rpos / lpos / window / look [V], running [V], envelopes in mxg_envgen_render's layout,
// stages_h / stages_l [V][3][6]
int dyn_state(void *h, double *rring, double *lring, int32_t *rpos, int32_t *lpos, uint32_t *window, uint32_t *look,
              double *running, double *dst_h, int64_t *ist_h, double *dst_l, int64_t *ist_l, double *stages_h,
              double *stages_l) {
    Bank *b = (Bank *)h;
    const size_t V = b->d.size();
    for (size_t v = 0; v < V; v++) {
        maxiDynamics &d = *b->d[v];
        for (size_t i = 0; i < d.rms.buf.size(); i++) rring[i * V + v] = d.rms.buf.buf[i];
        for (size_t i = 0; i < d.lookAheadDelay.size(); i++) lring[i * V + v] = d.lookAheadDelay.buf[i];
        rpos[v] = (int32_t)d.rms.buf.idx;
        lpos[v] = (int32_t)d.lookAheadDelay.idx;
        window[v] = (uint32_t)d.rms.windowSize;
        look[v] = (uint32_t)d.lookAheadSize;
        running[v] = d.rms.runningRMS;
        dump_env(d.arEnvHigh, V, v, dst_h, ist_h, stages_h + v * 18);
        dump_env(d.arEnvLow, V, v, dst_l, ist_l, stages_l + v * 18);
    }
    return 0;
}

// maxiRMS alone
void *rms_new(size_t V, int sr, double max_ms, double window_ms) {
    RmsBank *b = new RmsBank;
    maxiSettings::sampleRate = sr;
    for (size_t v = 0; v < V; v++) {
        maxiRMS *r = new (std::calloc(1, sizeof(maxiRMS))) maxiRMS();
        r->setup(max_ms, window_ms);
        b->r.push_back(r);
    }
    return b;
}
void rms_free(void *h) {
    RmsBank *b = (RmsBank *)h;
    for (maxiRMS *o : b->r) {
        o->~maxiRMS();
        std::free(o);
    }
    delete b;
}
void rms_set_window(void *h, size_t v, double ms) { ((RmsBank *)h)->r[v]->setWindowSize(ms); }
int rms_play(void *h, size_t N, const double *in, double *out) {
    RmsBank *b = (RmsBank *)h;
    const size_t V = b->r.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) out[n * V + v] = b->r[v]->play(in[n * V + v]);
    return 0;
}
int64_t rms_cap(void *h) { return (int64_t)((RmsBank *)h)->r[0]->buf.size(); }
int rms_state(void *h, double *ring, int32_t *pos, uint32_t *window, double *running) {
    RmsBank *b = (RmsBank *)h;
    const size_t V = b->r.size();
    for (size_t v = 0; v < V; v++) {
        maxiRMS &r = *b->r[v];
        for (size_t i = 0; i < r.buf.size(); i++) ring[i * V + v] = r.buf.buf[i];
        pos[v] = (int32_t)r.buf.idx;
        window[v] = (uint32_t)r.windowSize;
        running[v] = r.runningRMS;
    }
    return 0;
}

// maxiEnvGen::setupASR(10, 10) + setTime(index, ms): the [3][6] table afterwards, and setTime's return value
int envgen_set_time(int sr, double attack, double release, size_t index, double ms, double *stages) {
    maxiSettings::sampleRate = sr;
    maxiEnvGen *e = new (std::calloc(1, sizeof(maxiEnvGen))) maxiEnvGen();
    e->setupASR(attack, release);
    const int err = e->setTime(index, ms);
    for (size_t i = 0; i < e->stages.size(); i++) {
        double *st = stages + 6 * i;
        st[0] = e->stages[i].startlevel; st[1] = e->stages[i].endlevel; st[2] = e->stages[i].gradient;
        st[3] = e->stages[i].curve; st[4] = (double)e->stages[i].length; st[5] = e->stages[i].hold;
    }
    e->~maxiEnvGen();
    std::free(e);
    return err;
}

}  // extern "C"
