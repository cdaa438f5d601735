// tests/patches/analysis_host_patch.cpp -- the time-domain analysis classes alone, in the reference's plugin form:
// maxiZeroCrossingDetector, maxiZeroCrossingRate (its ring sized at a sample rate of 2000, so that it wraps inside the run, and
// a second one whose window is shortened mid-stream), maxiEnvelopeFollower and maxiEnvelopeFollowerF (attack and release set
// apart), and maxiSampleAndHold (a fixed, a moving and a zero hold time), driven by signals that are plain arithmetic.  Nothing
// here touches the device: these classes are host value types in the reference and in include/maximilian.h, so the stream is
// the same bits with either header on any machine (tests/test_analysis_dropin_cpu.py; tests/golden/analysis.npz["host_patch"]
// is the reference's).  maxiPoll owns a maxiOsc and therefore lives in analysis_patch.cpp.
#include "maximilian.h"

maxiZeroCrossingDetector zxd;
maxiZeroCrossingRate *zcrA, *zcrB;
maxiEnvelopeFollower follow, *followLate;
maxiEnvelopeFollowerF followF;
maxiSampleAndHold sahA, sahB, sahC;
double phaseA = 0, phaseB = 0.5, lfo = 0;
long frame = 0;

void setup() {
    follow.setAttack(3);      // (at the sample rate of construction, 44100)
    follow.setRelease(40);
    maxiSettings::sampleRate = 2000;
    zcrA = new maxiZeroCrossingRate;  // rings of 2000 slots
    zcrB = new maxiZeroCrossingRate;
    followLate = new maxiEnvelopeFollower;  // setAttack(100), setRelease(100) at 2000
    followF.setAttack(1.5f);
    followF.setRelease(25);
}

void play(double *output) {
    const double sr = (double)maxiSettings::sampleRate;
    phaseA += (40.0 + 0.02 * (double)(frame < 4000 ? frame : 8000 - frame)) / sr;  // 40 -> 120 -> 40 Hz and on down
    if (phaseA >= 1.0) phaseA -= 1.0;
    phaseB += 211.0 / sr;
    if (phaseB >= 1.0) phaseB -= 1.0;
    lfo += 3.0 / sr;
    if (lfo >= 1.0) lfo -= 2.0;
    const double saw = 2.0 * phaseA - 1.0;
    const double tri = (phaseB < 0.5 ? 4.0 * phaseB - 1.0 : 3.0 - 4.0 * phaseB) * (0.5 + 0.5 * lfo * lfo);
    const double sig = frame % 1000 < 40 ? 0.0 : saw * (1.0 - 0.5 * lfo);  // runs of exact zeros
    const double rateA = zcrA->play(sig);
    if (frame == 5000) maxiSettings::sampleRate = 1500;  // the second rate's window shrinks over its filled ring for one call...
    const double rateB = zcrB->play(tri);
    maxiSettings::sampleRate = 2000;                     // ...and is back at the ring's size for the next call
    const double level = follow.play(sig) + followLate->play(tri);
    const float levelF = followF.play((float)tri);
    const double held = sahA.sah(saw, 2.5) + 0.001 * sahB.sah(tri, 10.0 + 8.0 * lfo) + 1e-6 * sahC.sah(sig + 0.75, 0);
    output[0] = level + (double)levelF * 0.5;
    output[1] = rateA + 0.001 * rateB + 1e-5 * (zxd.zx(tri - 0.2) ? 1.0 : 0.0) + 1e-2 * held;
    frame++;
}
