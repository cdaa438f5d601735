// tools/gen/grainpool_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiTimeStretch / maxiPitchShift / maxiStretch (src/libs/maxiGrains.h): tools/gen/gen_golden_grainpool.py compiles it, together
// with the UNMODIFIED reference sources, into a shared library in a temporary directory and drives it to write
// tests/golden/grainpool.npz.  One object per stream, each with its own maxiSample.  The grain code's rand() is routed to the draws
// the caller supplies per stream, as oracle/ref_harness.cpp does; protected members are read through -fno-access-control.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "maximilian.h"

struct GpRnd {
    const int32_t *q = nullptr;
    size_t n = 0, i = 0;
    int underrun = 0;
};
static GpRnd *g_rnd = nullptr;
static int gp_ref_rand() {
    if (!g_rnd || !g_rnd->q) return 0;
    if (g_rnd->i >= g_rnd->n) {
        g_rnd->underrun = 1;
        return 0;
    }
    return g_rnd->q[g_rnd->i++];
}
#define rand gp_ref_rand
#include "libs/maxiGrains.h"
#undef rand

struct GpStream {
    GpRnd rnd;
    long long minIdx = 1LL << 60, maxIdx = -1, maxLive = 0, births = 0, deaths = 0, wrappedGrains = 0;
    size_t len = 0;
    virtual ~GpStream() {}
    virtual void setSample(maxiSample *s) = 0;
    virtual double play(int mode, double a, double b, double pm, double grainLength, int overlaps) = 0;
    virtual void state(double *st3) = 0;
    virtual void setPosition(double raw) = 0;
    virtual void setLoopStart(double v) {}
    virtual void setLoopEnd(double v) {}
    virtual void loop(uint64_t *l3) { l3[0] = l3[1] = l3[2] = 0; }
    virtual grainList &grains() = 0;
    virtual size_t dumpGrains(double *g4x8) = 0;
};

template <typename F, typename Obj>
struct GpStreamT : GpStream {
    Obj o;
    explicit GpStreamT(maxiSample *s) : o(s) { len = s->getLength(); }
    grainList &grains() override { return o.grainPlayer->grains; }
    void note(long long idx) {
        if (idx < minIdx) minIdx = idx;
        if (idx > maxIdx) maxIdx = idx;
    }
    // what the next play() of every live grain reads (:224-236), restated here only to CHECK the indices
    void before() {
        for (maxiGrainBase *gb : grains()) {
            maxiGrain<F> *g = static_cast<maxiGrain<F> *>(gb);
            double pos = g->pos + g->inc;
            bool w = false;
            if (pos >= (double)len) { pos -= len; w = true; } else if (pos < 0) { pos += len; w = true; }
            if (w) wrappedGrains++;
            const long a = (long)floor(pos);
            long b = a + 1;
            if (b >= (long)len) b = 0;
            note(a);
            note(b);
        }
    }
    void after(size_t liveBefore) {
        const size_t live = grains().size();
        // a grain born in this call has sampleIdx == 1 now: its first read was at floor(pos)
        for (maxiGrainBase *gb : grains()) {
            maxiGrain<F> *g = static_cast<maxiGrain<F> *>(gb);
            if (g->sampleIdx == 1) {
                births++;
                const long a = (long)floor(g->pos);
                note(a);
                note(a + 1 >= (long)len ? 0 : a + 1);
            }
        }
        (void)liveBefore;
        if ((long long)live > maxLive) maxLive = (long long)live;
    }
    size_t dumpGrains(double *g) override {
        size_t k = 0;
        for (maxiGrainBase *gb : grains()) {
            maxiGrain<F> *gr = static_cast<maxiGrain<F> *>(gb);
            if (k < 8) {
                g[0 * 8 + k] = gr->pos;
                g[1 * 8 + k] = gr->inc;
                g[2 * 8 + k] = (double)gr->sampleIdx;
                g[3 * 8 + k] = (double)gr->sampleDur;
            }
            k++;
        }
        return k;
    }
    double step(int mode, double a, double b, double pm, double grainLength, int overlaps);
    double play(int mode, double a, double b, double pm, double grainLength, int overlaps) override {
        g_rnd = &rnd;
        before();
        const size_t lb = grains().size();
        const double v = step(mode, a, b, pm, grainLength, overlaps);
        // deaths: live before + born - live after
        size_t born = 0;
        for (maxiGrainBase *gb : grains())
            if (static_cast<maxiGrain<F> *>(gb)->sampleIdx == 1) born++;
        deaths += (long long)(lb + born - grains().size());
        after(lb);
        g_rnd = nullptr;
        return v;
    }
    void setSample(maxiSample *s) override {
        o.setSample(s);
        len = s->getLength();
    }
    void state(double *st) override;
    void setPosition(double raw) override { o.position = raw; }
    void setLoopStart(double v) override;
    void setLoopEnd(double v) override;
    void loop(uint64_t *l3) override;
};

#define GP_TS(F) GpStreamT<F, maxiTimeStretch<F>>
#define GP_ST(F) GpStreamT<F, maxiStretch<F>>
#define GP_PS(F) GpStreamT<F, maxiPitchShift<F>>
#define GP_DEFINE(F)                                                                                                              \
    template <> double GP_TS(F)::step(int mode, double a, double b, double pm, double gl, int ov) {                             \
        return mode == 0 ? o.play(a, gl, ov, pm) : o.playAtPosition(a, gl, ov);                                                  \
    }                                                                                                                             \
    template <> double GP_ST(F)::step(int mode, double a, double b, double pm, double gl, int ov) {                             \
        return mode == 1 ? o.play(a, b, gl, ov, pm) : o.playAtPosition(a, b, gl, ov);                                            \
    }                                                                                                                             \
    template <> double GP_PS(F)::step(int mode, double a, double b, double pm, double gl, int ov) { return o.play(a, gl, ov, pm); } \
    template <> void GP_TS(F)::state(double *st) { st[0] = o.position; st[1] = o.looper; st[2] = o.randomOffset; }              \
    template <> void GP_ST(F)::state(double *st) { st[0] = o.position; st[1] = o.looper; st[2] = o.randomOffset; }              \
    template <> void GP_PS(F)::state(double *st) { st[0] = o.position; st[1] = (double)o.cycles; st[2] = o.randomOffset; }      \
    template <> void GP_TS(F)::setLoopStart(double) {}                                                                           \
    template <> void GP_TS(F)::setLoopEnd(double) {}                                                                             \
    template <> void GP_TS(F)::loop(uint64_t *l) { l[0] = l[1] = l[2] = 0; }                                                     \
    template <> void GP_PS(F)::setLoopStart(double) {}                                                                           \
    template <> void GP_PS(F)::setLoopEnd(double) {}                                                                             \
    template <> void GP_PS(F)::loop(uint64_t *l) { l[0] = l[1] = l[2] = 0; }                                                     \
    template <> void GP_ST(F)::setLoopStart(double v) { o.setLoopStart(v); }                                                     \
    template <> void GP_ST(F)::setLoopEnd(double v) { o.setLoopEnd(v); }                                                         \
    template <> void GP_ST(F)::loop(uint64_t *l) { l[0] = o.loopStart; l[1] = o.loopEnd; l[2] = o.loopLength; }

GP_DEFINE(hannWinFunctor)
GP_DEFINE(rectWinFunctor)
GP_DEFINE(gaussianWinFunctor)

template <typename F>
static GpStream *make(int mode, maxiSample *s) {
    if (mode == 0 || mode == 2) return new GP_TS(F)(s);
    if (mode == 3) return new GP_PS(F)(s);
    return new GP_ST(F)(s);
}

extern "C" {

maxiSample *gp_sample_new(const double *data, size_t n) {
    maxiSettings::setup(44100, 2, 1024);
    maxiSample *s = new maxiSample;
    std::vector<double> v(data, data + n);
    s->setSample(v);
    return s;
}
void gp_sample_free(maxiSample *s) { delete s; }

// window: 0 hann, 3 rect, 8 gaussian (the kinds of mxg_grain_plan_create)
GpStream *gp_new(int mode, int window, maxiSample *s, const int32_t *rnd, size_t rn) {
    GpStream *g = window == 0 ? make<hannWinFunctor>(mode, s) : window == 3 ? make<rectWinFunctor>(mode, s) : make<gaussianWinFunctor>(mode, s);
    g->rnd.q = rnd;
    g->rnd.n = rn;
    return g;
}
void gp_free(GpStream *g) { delete g; }
void gp_set_sample(GpStream *g, maxiSample *s) { g->setSample(s); }
void gp_set_position_raw(GpStream *g, double raw) { g->setPosition(raw); }
void gp_set_loop_start(GpStream *g, double v) { g->setLoopStart(v); }
void gp_set_loop_end(GpStream *g, double v) { g->setLoopEnd(v); }

// n calls; a, b, pm: one value per call.  pos [n]: `position` after every call.
void gp_run(GpStream *g, int mode, size_t n, const double *a, const double *b, const double *pm, double grainLength, int overlaps, double *out,
            double *pos) {
    double st[3];
    for (size_t i = 0; i < n; i++) {
        out[i] = g->play(mode, a[i], b ? b[i] : 0.0, pm ? pm[i] : 0.0, grainLength, overlaps);
        g->state(st);
        pos[i] = st[0];
    }
}

// st [3], gst [4][8], loop [3], stats [8]: min / max read index since the call before, most live grains, births, deaths, grain wraps, rand underrun, draws used
size_t gp_state(GpStream *g, double *st, double *gst, uint64_t *loop, long long *stats) {
    g->state(st);
    for (int i = 0; i < 32; i++) gst[i] = 0.0;
    const size_t k = g->dumpGrains(gst);
    g->loop(loop);
    stats[0] = g->minIdx; stats[1] = g->maxIdx; stats[2] = g->maxLive; stats[3] = g->births; stats[4] = g->deaths;
    stats[5] = g->wrappedGrains; stats[6] = g->rnd.underrun; stats[7] = (long long)g->rnd.i;
    g->minIdx = 1LL << 60;  // the index range is per piece (the slot may change between two)
    g->maxIdx = -1;
    return k;
}

void gp_window(int window, int length, double *w) {
    for (int i = 0; i < length; i++)
        w[i] = window == 0 ? hannWinFunctor()(length, i) : window == 3 ? rectWinFunctor()(length, i) : gaussianWinFunctor()(length, i);
}

}  // extern "C"
