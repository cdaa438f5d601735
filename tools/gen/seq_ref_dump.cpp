// tools/gen/seq_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiRatioSeq / maxiStep / maxiCounter / maxiIndex / maxiZXToPulse / maxiTrigger: tools/gen/gen_golden_seq.py compiles it,
// together with the UNMODIFIED reference sources, into a shared library in a temporary directory and drives it block by block
// to write tests/golden/seq.npz.
//
// V sets of objects live side by side and are called sample-major, as a patch with V sequencers calls them.  A fused voice is
// clock (maxiOsc::phasor) -> maxiRatioSeq -> playValues | maxiStep::pull -> maxiZXToPulse::play.  playValues does not return
// its trigger, so the trigger comes from a second maxiRatioSeq that is fed the same phase through playTrig (its prevPhase /
// first are the same by construction; the state that is dumped is the playValues object's).  State is read through
// -fno-access-control, in the layouts of include/maxigpu.h.
#include <cstdint>
#include <vector>

#include "maximilian.h"

namespace {

struct Voice {
    maxiOsc clock;
    maxiRatioSeq rseq, rtrig;
    maxiStep step;
    maxiZXToPulse pulse;
};
struct Bank {
    std::vector<Voice> v;
};
struct SigVoice {
    maxiTrigger zx;
    maxiCounter counter;
    maxiStep step;
    maxiIndex index;
    maxiZXToPulse pulse;
};
struct SigBank {
    std::vector<SigVoice> v;
};

std::vector<double> row(const double *tab, const int32_t *len, size_t L, int r) {
    return std::vector<double>(tab + (size_t)r * L, tab + (size_t)r * L + len[r]);
}

}  // namespace

extern "C" {

void seq_set_rate(int sr) { maxiSettings::sampleRate = sr; }

void *seq_new(size_t V) {
    Bank *b = new Bank;
    b->v.resize(V);
    return b;
}
void seq_free(void *h) { delete (Bank *)h; }

// freq [V] (internal clock; fps = 1: [N][V]) or phase [N][V]; mode 0 playValues, 1 maxiStep::pull, -1 neither
void seq_play(void *h, size_t N, const double *freq, int fps, const double *phase, const double *times, const int32_t *len,
              size_t L, const int32_t *pat, int mode, const double *values, const int32_t *vlen, size_t LV, const int32_t *vpat,
              const double *step, const double *hold, int want_gate, double *trig, double *val, double *gate, double *phase_out) {
    Bank *b = (Bank *)h;
    const size_t V = b->v.size();
    for (size_t v = 0; v < V; v++) {
        Voice &o = b->v[v];
        std::vector<double> t = row(times, len, L, pat[v]);
        std::vector<double> x = mode >= 0 ? row(values, vlen, LV, vpat[v]) : std::vector<double>();
        for (size_t n = 0; n < N; n++) {
            const double ph = freq ? o.clock.phasor(fps ? freq[n * V + v] : freq[v]) : phase[n * V + v];
            double tr;
            if (mode == 0) {
                val[n * V + v] = o.rseq.playValues(ph, t, x);
                tr = o.rtrig.playTrig(ph, t);
            } else {
                tr = o.rseq.playTrig(ph, t);
                if (mode == 1) val[n * V + v] = o.step.pull(tr, x, step[v]);
            }
            trig[n * V + v] = tr;
            if (want_gate) gate[n * V + v] = o.pulse.play(tr, hold[v]);
            if (phase_out) phase_out[n * V + v] = ph;
        }
    }
}

void seq_state(void *h, double *dst, int64_t *ist, double *clk) {
    Bank *b = (Bank *)h;
    const size_t V = b->v.size();
    for (size_t v = 0; v < V; v++) {
        Voice &o = b->v[v];
        clk[v] = o.clock.phase;
        dst[v] = o.rseq.prevPhase;
        dst[V + v] = o.step.trig.previousValue;
        dst[2 * V + v] = o.step.index;
        dst[3 * V + v] = o.pulse.trig.previousValue;
        dst[4 * V + v] = o.pulse.holdCounter;
        ist[v] = o.rseq.first;
        ist[V + v] = (int64_t)o.rseq.counter;
        ist[2 * V + v] = (int64_t)o.rseq.lengthOfValues;
        ist[3 * V + v] = o.step.trig.firstTrigger;
        ist[4 * V + v] = o.step.first;
        ist[5 * V + v] = o.pulse.trig.firstTrigger;
    }
}

void *sig_new(size_t V) {
    SigBank *b = new SigBank;
    b->v.resize(V);
    return b;
}
void sig_free(void *h) { delete (SigBank *)h; }

// kind: 0 onZX, 1 count, 2 maxiStep::pull, 3 maxiIndex::pull, 4 maxiZXToPulse::play (MXG_SEQ_* of include/maxigpu.h)
void sig_play(void *h, int kind, size_t N, const double *in, const double *in2, const double *values, const int32_t *vlen,
              size_t LV, const int32_t *vpat, const double *par, double *out) {
    SigBank *b = (SigBank *)h;
    const size_t V = b->v.size();
    for (size_t v = 0; v < V; v++) {
        SigVoice &o = b->v[v];
        std::vector<double> x = (kind == 2 || kind == 3) ? row(values, vlen, LV, vpat[v]) : std::vector<double>();
        for (size_t n = 0; n < N; n++) {
            const double a = in[n * V + v];
            double y;
            if (kind == 0) y = o.zx.onZX(a);
            else if (kind == 1) y = o.counter.count(a, in2[n * V + v]);
            else if (kind == 2) y = o.step.pull(a, x, par[v]);
            else if (kind == 3) y = o.index.pull(a, in2[n * V + v], x);
            else y = o.pulse.play(a, par[v]);
            out[n * V + v] = y;
        }
    }
}

void sig_state(void *h, int kind, double *dst, int64_t *ist) {
    SigBank *b = (SigBank *)h;
    const size_t V = b->v.size();
    for (size_t v = 0; v < V; v++) {
        SigVoice &o = b->v[v];
        double d[3] = {0, 0, 0};
        int64_t f[2] = {0, 0};
        if (kind == 0) { d[0] = o.zx.previousValue; f[0] = o.zx.firstTrigger; }
        else if (kind == 1) {
            d[0] = o.counter.value; d[1] = o.counter.inctrig.previousValue; d[2] = o.counter.rstrig.previousValue;
            f[0] = o.counter.inctrig.firstTrigger; f[1] = o.counter.rstrig.firstTrigger;
        } else if (kind == 2) {
            d[0] = o.step.trig.previousValue; d[1] = o.step.index; f[0] = o.step.trig.firstTrigger; f[1] = o.step.first;
        } else if (kind == 3) {
            d[0] = o.index.trig.previousValue; d[1] = o.index.value; f[0] = o.index.trig.firstTrigger;
        } else {
            d[0] = o.pulse.trig.previousValue; d[1] = o.pulse.holdCounter; f[0] = o.pulse.trig.firstTrigger;
        }
        for (int k = 0; k < 3; k++) dst[k * V + v] = d[k];
        for (int k = 0; k < 2; k++) ist[k * V + v] = f[k];
    }
}

}  // extern "C"
