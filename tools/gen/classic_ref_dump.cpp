// tools/gen/classic_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's maxiDyn,
// maxiEnvelope, maxiLagExp<double>, maxiMap and maxiConvert: tools/gen/gen_golden_classic.py compiles it, together with the
// UNMODIFIED reference sources, into a shared library in a temporary directory and drives it block by block to write
// tests/golden/classic.npz.
//
// V objects of a class live side by side and are called sample-major; their state is read and written in the layouts of
// include/maxigpu.h.  The objects are value-initialised (all members zero: the library's static-storage rule).  The envelope's
// segment vectors are padded with three entries behind the count'th, so that the reference's own reads past the count
// stay inside the vector; the generator checks that no output changes with the padding's value.
#include <cstdint>
#include <vector>

#include "maximilian.h"

extern "C" {

void cls_set_rate(int sr) { maxiSettings::sampleRate = sr; }

void *cls_dyn_new(size_t V) {
    auto *d = new std::vector<maxiDyn>(V);
    for (auto &x : *d) x = maxiDyn();  // value-initialised: every member zero
    return d;
}
void cls_dyn_free(void *h) { delete (std::vector<maxiDyn> *)h; }

// in, thr, att, rel [N][V]; holdtime [V]
// trace [N][V] (the generator's checks): attackphase + 2 * holdphase + 4 * releasephase after each call; level: amplitude
void cls_dyn_gate(void *h, size_t N, const double *in, const double *thr, const int64_t *holdtime, const double *att, const double *rel, double *out,
                  int32_t *trace, double *level) {
    std::vector<maxiDyn> &D = *(std::vector<maxiDyn> *)h;
    const size_t V = D.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            out[n * V + v] = D[v].gate(in[n * V + v], thr[n * V + v], (long)holdtime[v], att[n * V + v], rel[n * V + v]);
            trace[n * V + v] = D[v].attackphase + 2 * D[v].holdphase + 4 * D[v].releasephase;
            level[n * V + v] = D[v].amplitude;
        }
}

// level [N][V]: currentRatio after each call
void cls_dyn_compressor(void *h, size_t N, const double *in, const double *ratio, const double *thr, const double *att, const double *rel, double *out,
                        double *level) {
    std::vector<maxiDyn> &D = *(std::vector<maxiDyn> *)h;
    const size_t V = D.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            out[n * V + v] = D[v].compressor(in[n * V + v], ratio[n * V + v], thr[n * V + v], att[n * V + v], rel[n * V + v]);
            level[n * V + v] = D[v].currentRatio;
        }
}

// the setters of voice v (attack / release in ms), then compress() reads the members
void cls_dyn_set(void *h, size_t v, double ratio, double threshold, double attack_ms, double release_ms) {
    maxiDyn &d = (*(std::vector<maxiDyn> *)h)[v];
    d.setRatio(ratio);
    d.setThreshold(threshold);
    d.setAttack(attack_ms);
    d.setRelease(release_ms);
}
// par [4]: the members ratio, threshold, attack, release of voice v
void cls_dyn_members(void *h, size_t v, double *par) {
    maxiDyn &d = (*(std::vector<maxiDyn> *)h)[v];
    par[0] = d.ratio; par[1] = d.threshold; par[2] = d.attack; par[3] = d.release;
}
void cls_dyn_compress(void *h, size_t N, const double *in, double *out, double *level) {
    std::vector<maxiDyn> &D = *(std::vector<maxiDyn> *)h;
    const size_t V = D.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            out[n * V + v] = D[v].compress(in[n * V + v]);
            level[n * V + v] = D[v].currentRatio;
        }
}
// dst [3][V] = amplitude, currentRatio, output; ist [4][V] = holdcount, attackphase, holdphase, releasephase
void cls_dyn_state(void *h, double *dst, int64_t *ist) {
    std::vector<maxiDyn> &D = *(std::vector<maxiDyn> *)h;
    const size_t V = D.size();
    for (size_t v = 0; v < V; v++) {
        dst[v] = D[v].amplitude; dst[V + v] = D[v].currentRatio; dst[2 * V + v] = D[v].output;
        ist[v] = D[v].holdcount; ist[V + v] = D[v].attackphase; ist[2 * V + v] = D[v].holdphase; ist[3 * V + v] = D[v].releasephase;
    }
}

struct EnvBank {
    std::vector<maxiEnvelope> e;
    std::vector<std::vector<double>> seg;
    std::vector<int> count;
};
// seg [S][V], count [V]; pad: the value of the three entries behind the count'th
void *cls_env_new(size_t V, size_t S, const double *seg, const int32_t *count, double pad) {
    auto *b = new EnvBank;
    b->e.resize(V);
    b->seg.resize(V);
    b->count.assign(count, count + V);
    for (size_t v = 0; v < V; v++) {
        b->e[v] = maxiEnvelope();
        b->e[v].period = b->e[v].output = b->e[v].startval = b->e[v].currentval = b->e[v].nextval = b->e[v].amplitude = 0;
        b->e[v].isPlaying = b->e[v].valindex = 0;
        for (int i = 0; i < count[v]; i++) b->seg[v].push_back(seg[(size_t)i * V + v]);
        for (int i = 0; i < 3; i++) b->seg[v].push_back(pad);
    }
    return b;
}
void cls_env_free(void *h) { delete (EnvBank *)h; }
void cls_env_trigger(void *h, size_t v, int index, double amp) { ((EnvBank *)h)->e[v].trigger(index, amp); }
// trig [N][V] or null: a non-zero value triggers (index[v], amp[v]) before that sample's line()
void cls_env_line(void *h, size_t N, const double *trig, const int32_t *index, const double *amp, double *out, int32_t *valindex) {
    EnvBank &b = *(EnvBank *)h;
    const size_t V = b.e.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            if (trig && trig[n * V + v] != 0.0) b.e[v].trigger(index[v], amp[v]);
            out[n * V + v] = b.e[v].line(b.count[v], b.seg[v]);
            valindex[n * V + v] = b.e[v].valindex;
        }
}
// dst [2][V] = amplitude, startval; ist [2][V] = valindex, isPlaying
void cls_env_state(void *h, double *dst, int32_t *ist) {
    EnvBank &b = *(EnvBank *)h;
    const size_t V = b.e.size();
    for (size_t v = 0; v < V; v++) {
        dst[v] = b.e[v].amplitude; dst[V + v] = b.e[v].startval;
        ist[v] = b.e[v].valindex; ist[V + v] = b.e[v].isPlaying;
    }
}

void *cls_lag_new(size_t V, const double *alpha, const double *val) {
    auto *l = new std::vector<maxiLagExp<double>>;
    for (size_t v = 0; v < V; v++) l->push_back(maxiLagExp<double>(alpha[v], val[v]));
    return l;
}
void cls_lag_free(void *h) { delete (std::vector<maxiLagExp<double>> *)h; }
void cls_lag_set_alpha(void *h, size_t v, double alpha) { (*(std::vector<maxiLagExp<double>> *)h)[v].setAlpha(alpha); }
void cls_lag_add(void *h, size_t N, const double *in, double *out) {
    std::vector<maxiLagExp<double>> &L = *(std::vector<maxiLagExp<double>> *)h;
    const size_t V = L.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            L[v].addSample(in[n * V + v]);
            out[n * V + v] = L[v].value();
        }
}
// par [2][V] = alpha, alphaReciprocal; val [V]
void cls_lag_state(void *h, double *par, double *val) {
    std::vector<maxiLagExp<double>> &L = *(std::vector<maxiLagExp<double>> *)h;
    const size_t V = L.size();
    for (size_t v = 0; v < V; v++) { par[v] = L[v].getAlpha(); par[V + v] = L[v].getAlphaReciprocal(); val[v] = L[v].value(); }
}

// mode: include/maxigpu.h MXG_MAP_*; x [n], r [4][n]
void cls_map(int mode, size_t n, const double *x, const double *r, double *out) {
    for (size_t i = 0; i < n; i++) switch (mode) {
            case 0: out[i] = maxiMap::linlin(x[i], r[i], r[n + i], r[2 * n + i], r[3 * n + i]); break;
            case 1: out[i] = maxiMap::linexp(x[i], r[i], r[n + i], r[2 * n + i], r[3 * n + i]); break;
            case 2: out[i] = maxiMap::explin(x[i], r[i], r[n + i], r[2 * n + i], r[3 * n + i]); break;
            case 3: out[i] = maxiMap::clamp(x[i], r[i], r[n + i]); break;
            case 4: out[i] = maxiConvert::ampToDbs(x[i]); break;
            default: out[i] = maxiConvert::dbsToAmp(x[i]); break;
        }
}

}  // extern "C"
