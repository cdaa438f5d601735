// tests/patches/fx_patch.cpp -- maxiFlanger and maxiChorus driven by maxiEnvGen ramps shaped like the reference's 23.Chorus and
// 24.Flanger examples (shorter ramps), on an oscillator source; a maxiFlanger copied inside a std::vector (value semantics).
// Built against include/maximilian.h as host/dropin_p7 (tests/test_gpu_fx_dropin.py) and, for tests/golden/fx.npz["patch"],
// against the reference sources by tools/gen/gen_golden_fx.py.
#include <vector>

#include "maximilian.h"

maxiOsc osc;
maxiFlanger flanger;
maxiChorus chorus;
maxiEnvGen delayEnv, fbEnv, speedEnv, cDelayEnv, cFbEnv, cSpeedEnv;
std::vector<maxiFlanger> flangers;
long frame = 0;

void setup() {
    delayEnv.setup({50, 1000, 10}, {60, 60}, {1, 1}, true);
    fbEnv.setup({0.8, 0.99, 0.8}, {90, 90}, {1, 1}, true);
    speedEnv.setup({0.1, 1, 0.1}, {150, 150}, {1, 1}, true);
    cDelayEnv.setup({10, 1000, 10}, {60, 60}, {1, 1}, true);
    cFbEnv.setup({0.2, 0.99, 0.2}, {90, 90}, {1, 1}, true);
    cSpeedEnv.setup({0.01, 10, 0.01}, {150, 150}, {1, 1}, true);
    flangers.resize(2);
}

void play(double *output) {
    const double w = osc.saw(110) * 0.5;
    const double a = flanger.flange(w, delayEnv.play(1), fbEnv.play(1), speedEnv.play(1), 1);
    const double b = chorus.chorus(w, cDelayEnv.play(1), cFbEnv.play(1), cSpeedEnv.play(1), 1);
    double c = flangers[0].flange(w, 30, 0.7, 3.0, 0.8) + flangers[1].flange(w, 200, 0.5, 0.5, 1.2);
    if (frame == 3000) flangers.push_back(flangers[0]);  // a copy (and a reallocation that copies the others)
    if (frame >= 3000) c += flangers[2].flange(w, 30, 0.7, 3.0, 0.8);
    output[0] = a + 0.25 * c;
    output[1] = b;
    frame++;
}
