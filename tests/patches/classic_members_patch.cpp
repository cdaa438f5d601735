// tests/patches/classic_members_patch.cpp -- touches every public member of the drop-in maxiDyn and maxiEnvelope the way a patch
// written against the reference may: the eight doubles, holdtime, holdcount and the three phases of maxiDyn, valindex and
// amplitude of maxiEnvelope with their getters and setters; both classes are copied, assigned and kept in arrays.  No device is
// needed (tests/test_classic_dropin_cpu.py compiles it against include/maximilian.h and, where the reference is present, against
// the reference, and runs the first build).
#include "maximilian.h"

maxiDyn dyns[3];
maxiEnvelope envs[2];
std::vector<double> segs = {0.5, 1.0, 0.0, 1.0};

void setup() {
    maxiDyn &d = dyns[0];
    d.input = 0.25; d.ratio = 3.0; d.currentRatio = 0.0; d.threshold = 0.3; d.output = 0.0; d.attack = 0.5; d.release = 0.99; d.amplitude = 0.0;
    d.holdtime = 4; d.holdcount = 0; d.attackphase = 0; d.holdphase = 0; d.releasephase = 0;
    d.setAttack(1.0); d.setRelease(2.0); d.setThreshold(0.35); d.setRatio(2.5);
    dyns[1] = d;            // assignment
    maxiDyn copy(dyns[1]);  // copy construction
    dyns[2] = copy;
    envs[0].setValindex(0);
    envs[0].setAmplitude(0.1);
    envs[0].trigger(envs[0].getValindex(), envs[0].getAmplitude());
    envs[1] = envs[0];
}

void play(double *output) {
    const double x = (double)((dyns[0].holdcount * 7 + envs[0].valindex) % 5) / 4.0 - 0.5;
    double a = dyns[0].gate(x, dyns[0].threshold, dyns[0].holdtime, dyns[0].attack, dyns[0].release) + dyns[1].compress(x) + dyns[2].compressor(x, 4.0);
    a += dyns[0].amplitude + dyns[1].currentRatio + dyns[1].output + (double)(dyns[0].attackphase + dyns[0].holdphase + dyns[0].releasephase);
    maxiEnvelope e(envs[1]);
    output[0] = a;
    output[1] = envs[0].line(4, segs) + e.line(4, segs) + envs[0].amplitude + (double)envs[0].valindex;
}
