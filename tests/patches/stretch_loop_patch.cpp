// tests/patches/stretch_loop_patch.cpp -- a patch in the reference's plugin form (void setup(); void play(double*);): one
// maxiStretch<hannWinFunctor> with loop points -- setLoopStart(0.25), setLoopEnd(0.5) -- played with a pitch and a timestretch that
// step every few thousand samples (a negative rate among them, so the position wraps at both ends of the loop), then driven through
// maxiStretch::playAtPosition with a position signal.  The scheduler's jitter comes from the process-wide rand() (L/maxiGrains.h:523).
// TEST INFRASTRUCTURE: compiled once against the reference's src/maximilian.h + src/libs/maxiGrains.h (tools/gen/
// gen_golden_grainpool.py -> the stream patch_sl of tests/golden/grainpool.npz) and once against include/maximilian.h +
// include/maxiGrains.h (host/Makefile dropin_sl).
#include "maximilian.h"
#include "maxiGrains.h"

maxiSample samp;
maxiStretch<hannWinFunctor> *st;
int n = 0;
const int kPlay = 9000;  // samples of play() before playAtPosition takes over

void setup() {
    vector<double> data(60000);
    for (int i = 0; i < 60000; i++)  // integer arithmetic only: a rough tone with a slow tremolo and some grit
        data[i] = ((((i * 37) % 401) - 200) / 300.0) * (0.5 + ((i / 2000) % 4) * 0.125) + (((i * 7919) % 2001) - 1000) / 20000.0;
    samp.setSample(data);
    st = new maxiStretch<hannWinFunctor>(&samp);
    st->setLoopStart(0.25);
    st->setLoopEnd(0.5);
    st->setPosition(0.3);
}

void play(double *output) {
    static const double rates[4] = {1.0, 0.5, -1.0, 2.0}, pitches[3] = {1.0, 1.5, 0.7};
    double w;
    if (n < kPlay)
        w = st->play(pitches[(n / 3000) % 3], rates[(n / 2000) % 4], 0.05, 2, 0.0);
    else
        w = st->playAtPosition(1.2, ((n * 3) % 1000) / 1024.0, 0.05, 3);
    output[0] = w;
    output[1] = st->getLoopEnd() == 30000 && st->loopStart == 15000 && st->loopLength == 15000 ? 0.5 * w : 0.0;
    n++;
}
