// tests/patches/drums_patch.cpp -- a patch in the reference's plugin form around maxiKick, maxiSnare, maxiHats and the maxiClock that
// triggers them: sixteenth notes at 375 bpm (a tick every 441 samples at 44 100 Hz), the kick on every tick, the snare on every second,
// the hats on every tick and a second hats object on every third.  In mid-stream: the second hats object becomes a COPY of the first
// (it continues from the same state, then goes its own way), a setter on the snare's public envelope, setCutoff / setResonance on
// the hats' public filter, and the public switches and scalars of the snare move.  output[0] sums snare and hats -- compares,
// + - * /, table reads and the rand() draws in call order: the reference's bits.  output[1] is the kick, whose sine is within 1 ULP.
// Built against include/ as host/dropin_dr; compiles against the reference as it stands (tests/test_drums_dropin_cpu.py).
#include "maximilian.h"
#include "maxiSynths.h"
#include "libs/maxiClock.h"

maxiKick kick;
maxiSnare snare;
maxiHats hats, hats2;
maxiClock drumClock;
long frame = 0;

void setup() {
    drumClock.setTicksPerBeat(4);
    drumClock.setTempo(1500);  // bps 100
    kick.setRelease(40);
    kick.setPitch(180);
    snare.setRelease(30);
    snare.envelope.setDecay(5);
    snare.cutoff = 3000;
    snare.resonance = 2;
    hats.setRelease(20);
    hats.useFilter = true;
    hats2.setRelease(10);
}

void play(double *output) {
    drumClock.ticker();
    if (drumClock.tick) {
        kick.trigger();
        if (drumClock.playHead % 2 == 0) snare.trigger();
        hats.trigger();
        if (drumClock.playHead % 3 == 0) hats2.trigger();
    }
    if (frame == 3000) hats2 = hats;  // a copy continues from the same state
    if (frame == 5000) {
        snare.envelope.setRelease(80);
        hats.filter.setCutoff(5000);
        hats.filter.setResonance(3);
    }
    if (frame == 7000) {
        kick.setUseDistortion(true);
        kick.setDistortion(2.0);
        snare.useDistortion = true;
        snare.distortion = 1.5;
        snare.useLimiter = true;
        snare.gain = 1.5;
        hats2.pitch = 9000;
        hats2.inverse = true;
    }
    const double k = kick.play();
    const double s = snare.play(), h = hats.play(), h2 = hats2.play();  // (the draws: snare, hats, hats2, every frame)
    output[0] = (s + h + h2) / 3.0;
    output[1] = k;
    frame++;
}
