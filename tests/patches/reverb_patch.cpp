// tests/patches/reverb_patch.cpp -- maxiSatReverb, maxiFreeVerb and maxiFreeVerbStereo behind an enveloped oscillator: both
// maxiFreeVerb overloads on one object with moving parameters that pass both clamps, playStereo into both output channels, copies
// made mid-stream and played beside their sources, and a std::vector of reverbs that grows (value semantics).
// Built against include/ as host/dropin_rv (tests/test_gpu_reverb_dropin.py) and, for tests/golden/reverb.npz["patch"], against
// the reference sources by tools/gen/gen_golden_reverb.py.
#include <vector>

#include "maximilian.h"
#include "maxiReverb.h"

maxiOsc osc, roomLfo, absLfo;
maxiEnv env;
maxiSatReverb sat;
maxiFreeVerb fv, fvCopy;
maxiFreeVerbStereo fvs, fvsCopy;
std::vector<maxiSatReverb> sats;
long frame = 0;

void setup() {
    env.setAttack(5);
    env.setDecay(50);
    env.setSustain(0.4);
    env.setRelease(300);
    sats.resize(2);
}

void play(double *output) {
    const int trig = (frame % 2000) < 300;
    const double w = osc.saw(110) * env.adsr(0.5, trig);
    const double room = roomLfo.sinewave(3.1) * 14.0 - 3.0;  // -17 .. 11: the comb weight leaves [0, 1] on both sides
    const double absorb = absLfo.triangle(1.7) * 1.4;        // -1.4 .. 1.4
    const double a = sat.play(w);
    const bool plain = (frame % 700) < 250;
    const double b = plain ? fv.play(w) : fv.play(w, room, absorb);
    double *st = fvs.playStereo(w, room, absorb);
    double l = st[0], r = st[1];
    double *ss = sats[0].playStereo(w * 0.5);
    l += ss[0];
    r += ss[1];
    const double c = sats[1].play(-w);
    if (frame == 2500) {
        fvCopy = fv;
        fvsCopy = fvs;
        sats.push_back(sats[1]);  // a copy, and a reallocation that copies the others
    }
    double d = 0.0, e = 0.0;
    if (frame >= 2500) {
        d = plain ? fvCopy.play(w) : fvCopy.play(w, room, absorb);  // = b
        e = fvsCopy.playStereo(w, 0.0, 0.0)[1] + sats[2].play(-w);  // = the right channel of fvs + c
    }
    output[0] = a + b + l + c;
    output[1] = r + d + e;
    frame++;
}
