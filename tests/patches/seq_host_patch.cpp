// tests/patches/seq_host_patch.cpp -- the sequencing classes alone, in the reference's plugin form: maxiRatioSeq (playTrig and
// playValues, with a value list whose length changes mid-stream), maxiStep (a fractional, a negative and an over-long step),
// maxiCounter, maxiIndex, maxiZXToPulse and maxiTrigger, driven by a clock that is plain arithmetic.  Nothing here touches
// the device: these classes are host value types in the reference and in include/maximilian.h, so the stream is the same bits
// with either header on any machine (tests/test_seq_host.py; tests/golden/seq.npz["host_patch"] is the reference's).
#include "maximilian.h"

maxiRatioSeq seqA, seqB, seqC;
maxiStep stepA, stepB, stepC;
maxiCounter counter;
maxiIndex picker;
maxiZXToPulse pulse;
maxiTrigger zx;
std::vector<double> ratios = {4, 4, 4, 1, 1, 1, 1}, odd = {33, 991, 13, 153};
std::vector<double> notes = {60, 62, 65, 67, 70, 72}, picks = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
double phaseA = 0, phaseB = 0.25, lfo = 0;
long frame = 0;

void setup() {}

void play(double *output) {
    const double sr = (double)maxiSettings::sampleRate;
    phaseA += 97.0 / sr;
    if (phaseA >= 1.0) phaseA -= 1.0;
    phaseB += (31.0 + 0.002 * (double)frame) / sr;
    if (phaseB >= 1.0) phaseB -= 1.0;
    lfo += 13.0 / sr;
    if (lfo >= 1.0) lfo -= 2.0;
    if (frame == 5000) notes = {48, 50, 53};  // playValues sees the new length
    const double trigA = seqA.playTrig(phaseA, {3, 3, 2});
    const double value = seqB.playValues(phaseB, ratios, notes);
    const double trigC = seqC.playTrig(phaseB, odd);
    const double a = stepA.pull(trigA, {40, 80, 170, 350, 900, 3888}, 0.5);
    const double b = stepB.pull(trigC, {1, 2, 3, 4}, -1);
    const double c = stepC.pull(trigA, {100, 200, 300}, 7);
    const double hits = counter.count(trigA, lfo);
    const double pick = picker.pull(trigC, lfo * 0.7 + 0.5, picks);
    const double gate = pulse.play(trigA, 37.5);
    output[0] = value + 1000.0 * a + 0.001 * b + 0.25 * gate + 1e6 * zx.onZX(lfo);
    output[1] = c + 0.01 * hits + 1e-4 * pick + 10000.0 * trigC;
    frame++;
}
