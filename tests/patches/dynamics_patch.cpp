// tests/patches/dynamics_patch.cpp -- a compressor demo in the reference's plugin form: an oscillator mix goes through
// maxiDynamics::compress (RMS detector, look-ahead on) whose threshold and ratio are moved by two looping maxiEnvGens; a second
// maxiDynamics in PEAK mode is side-chained from an LFO-gated signal with compandBelow.  One setter is called mid-stream and the
// PEAK object is copied mid-stream (the copy plays on, the source is left alone).  The PEAK detector holds no reference to its
// owner, so the copy is well defined in the reference too.
// Built against include/maximilian.h as host/dropin_p8 (tests/test_gpu_dyn_dropin.py) and, for tests/golden/dyn.npz["patch"],
// against the reference sources by tools/gen/gen_golden_dyn.py.
#include "maximilian.h"

maxiOsc saw1, saw2, tri, lfo, gateOsc;
maxiDynamics comp, duck, duck2;
maxiEnvGen threshEnv, ratioEnv;
long frame = 0;

void setup() {
    comp.setAttackHigh(20);
    comp.setReleaseHigh(10);
    comp.setLookAhead(2);
    comp.setRMSWindowSize(10);
    comp.setInputAnalyser(maxiDynamics::RMS);
    duck.setInputAnalyser(maxiDynamics::PEAK);
    duck.setAttackLow(5);
    duck.setReleaseLow(40);
    duck.setLookAhead(1);
    threshEnv.setup({-3, -40, -3}, {70, 50}, {1, 1}, true);
    ratioEnv.setup({8, 1, 0.3}, {90, 60}, {1, 1}, true);
}

void play(double *output) {
    const double swell = lfo.phasor(3);                                    // 0 .. 1, three times a second
    const double mix = (saw1.saw(110) * 0.4 + saw2.saw(164.5) * 0.3 + tri.triangle(55) * 0.3) * (0.02 + 0.98 * swell * swell);
    const double a = comp.compress(mix, threshEnv.play(1), ratioEnv.play(1), 5);
    if (frame == 4000) comp.setReleaseHigh(120);                           // a setter mid-stream
    const double gate = gateOsc.square(7) * 0.6 + 0.05;                    // the side chain: 0.65 / 0.05
    const double key = mix * gate;
    double b;
    if (frame < 6000) {
        b = duck.compandBelow(mix, key, -24, 3, 6);
        if (frame == 5999) duck2 = duck;                                   // a copy mid-stream
    } else {
        b = duck2.compandBelow(mix, key, -24, 3, 6);
    }
    output[0] = a;
    output[1] = b;
    frame++;
}
