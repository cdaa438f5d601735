// tests/patches/kuramoto_patch.cpp -- phase-coupled oscillator sets in the reference's plugin form.  A pair under strong
// coupling (K = 1900 at 44.1 kHz pulls two oscillators together within a few dozen samples), a set of seven under a weak,
// negative-going drift, and two asynchronous sets of three that stand for two machines on a network: each runs free on its last
// guess of the other's phases and, every 2000 samples, is told the other's own phase (setPhase) or all of them (setPhases).
// The pair's mix is mapped exponentially onto a pitch (maxiMap::linexp) and played by a maxiOsc::sawn, which is exact on the
// device, so channel 1 carries the reference's bits wherever channel 0 does.  Channel 0 is host arithmetic only: built with
// -DKURAMOTO_PATCH_NO_OSC the patch needs no device (tests/test_kuramoto_dropin_cpu.py; tests/golden/kuramoto.npz["patch"]).
// Built against include/maximilian.h as host/dropin_ku.
#include "maximilian.h"

maxiKuramotoOscillatorSet duo(2), seven(7);
maxiAsyncKuramotoOscillator here(3), there(3);
#ifndef KURAMOTO_PATCH_NO_OSC
maxiOsc tone;
#endif
long frame = 0;

void setup() {
    duo.setPhases({0.4, 3.3});
    seven.setPhases({0.1, 1.0, 1.9, 2.8, 3.7, 4.6, 5.5});
    here.setPhases({0.0, 2.0, 4.0});
    there.setPhases({3.0, 5.0, 1.0});
    seven.setPhase(6.2, 6);
}

void play(double *output) {
    const double both = duo.play(35.0, 1900.0);
    const double many = seven.play(-61.0, frame < 3000 ? 700.0 : -150.0);
    if (frame && frame % 2000 == 0) {
        if (frame % 4000 == 0) {  // everything the other side knows
            std::vector<double> a, b;
            for (size_t i = 0; i < here.size(); i++) {
                a.push_back(here.getPhase(i));
                b.push_back(there.getPhase(i));
            }
            here.setPhases(b);
            there.setPhases(a);
        } else {  // the other side's own oscillator only
            const double mine = here.getPhase(0), yours = there.getPhase(0);
            here.setPhase(yours, 1);
            there.setPhase(mine, 1);
        }
    }
    const double local = here.play(90.0, 4000.0), remote = there.play(93.0, 4000.0);
    const double pitch = maxiMap::linexp(both, 0.0, TWOPI, 110.0, 880.0);
    output[0] = 0.001 * pitch + many + 0.25 * (local - remote) + 0.125 * (double)duo.size() * duo.getPhase(1);
#ifndef KURAMOTO_PATCH_NO_OSC
    output[1] = tone.sawn(pitch);
#else
    output[1] = 0.0;
#endif
    frame++;
}
