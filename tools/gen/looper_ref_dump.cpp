// tools/gen/looper_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiSample::loopRecord / play / playLoop / trigger / normalise: tools/gen/gen_golden_looper.py compiles it, together with the
// UNMODIFIED reference sources, into a shared library in a temporary directory and drives it to write tests/golden/looper.npz.
// Private members (recordPosition, loopRecordLag.val) are read and set through -fno-access-control.
#include <cstdint>
#include <cstring>
#include <vector>

#include "maximilian.h"

struct LpBank {
    std::vector<maxiSample *> s;
};

extern "C" {

LpBank *lp_new(size_t R) {
    LpBank *b = new LpBank;
    for (size_t r = 0; r < R; r++) b->s.push_back(new maxiSample);
    return b;
}

void lp_free(LpBank *b) {
    for (maxiSample *s : b->s) delete s;
    delete b;
}

void lp_set_sample(LpBank *b, size_t r, const double *data, size_t n) {
    std::vector<double> v(data, data + n);
    b->s[r]->setSample(v);
}

void lp_set_heads(LpBank *b, size_t r, double recordPosition, double position) {
    b->s[r]->recordPosition = recordPosition;
    b->s[r]->position = position;
}

void lp_trigger(LpBank *b, size_t r) { b->s[r]->trigger(); }

// n samples of every slot: loopRecord, then play() (mode 0) or playLoop (mode 2).  in, enable, out [n][R]; the enable goes in as
// the double it is (C++ converts it to the bool parameter).  recidx / playidx [n][R]: the elements the two heads were on.
void lp_run(LpBank *b, size_t n, const double *in, const double *enable, const double *mix, const double *start, const double *end, int mode,
            const double *pstart, const double *pend, double *out, int64_t *recidx, int64_t *playidx) {
    const size_t R = b->s.size();
    for (size_t r = 0; r < R; r++) {
        maxiSample &s = *b->s[r];
        for (size_t i = 0; i < n; i++) {
            const double lo = start[r] * s.amplitudes.size();
            recidx[i * R + r] = (int64_t)(s.recordPosition < lo ? lo : s.recordPosition);
            s.loopRecord(in[i * R + r], enable[i * R + r], mix[r], start[r], end[r]);
            if (mode == 0) {
                playidx[i * R + r] = (int64_t)s.position;
                out[i * R + r] = s.play();
            } else {
                out[i * R + r] = s.playLoop(pstart[r], pend[r]);
                playidx[i * R + r] = (int64_t)s.position;
            }
        }
    }
}

void lp_state(LpBank *b, double *recpos, double *lag, double *position) {
    for (size_t r = 0; r < b->s.size(); r++) {
        recpos[r] = b->s[r]->recordPosition;
        lag[r] = b->s[r]->loopRecordLag.val;
        position[r] = b->s[r]->position;
    }
}

size_t lp_content(LpBank *b, size_t r, double *dst) {
    memcpy(dst, b->s[r]->amplitudes.data(), b->s[r]->amplitudes.size() * sizeof(double));
    return b->s[r]->amplitudes.size();
}

void lp_normalise(LpBank *b, size_t r, double maxLevel) { b->s[r]->normalise(maxLevel); }

}  // extern "C"
