// tests/patches/analysis_patch.cpp -- an analysed voice in the reference's plugin form, after the graph of the reference's
// example 22.Analysis: two detuned maxiOsc::sawn under a slow phasor's ramp go through a maxiZeroCrossingRate, a
// maxiEnvelopeFollower and a maxiSampleAndHold, a maxiZeroCrossingDetector re-triggers a straight maxiEnvGen from the audio, and
// three maxiPoll print what they are given.  Every source is exact on the device (sawn, phasor, an envelope of curve 1 at
// constant frequencies; no sinewave), so the stream is the reference's bits (tests/test_gpu_analysis_dropin.py;
// tests/golden/analysis.npz["patch"]) and so is the text on stdout.  Built against include/maximilian.h as host/dropin_an.
#include "maximilian.h"

maxiOsc osc1, osc2, ramp, slow;
maxiEnvGen ping;
maxiZeroCrossingDetector zxd;
maxiZeroCrossingRate zcr;
maxiEnvelopeFollower follow;
maxiEnvelopeFollowerF followF;
maxiSampleAndHold sah;
maxiPoll poll1, poll2, poll3;

void setup() {
    ping.setup({0, 1, 0}, {2, 30}, {1, 1}, false, false);
    follow.setAttack(2);
    follow.setRelease(60);
}

void play(double *output) {
    double w = osc1.sawn(110) + osc2.sawn(223.3);
    w = w * (ramp.phasor(7) - 0.25);
    const double rate = poll1.poll(zcr.play(w), 30, "zcr: ", "");
    const double level = poll2.poll(follow.play(w), 30, "\t level: ", "");
    const double held = poll3.poll(sah.sah(w, 2.5), 30, "\t held: ");
    const double trig = zxd.zx(slow.phasor(13) - 0.5) ? 1.0 : 0.0;
    output[0] = level + 0.5 * (double)followF.play((float)held) + 0.125 * ping.play(trig);
    output[1] = rate + 0.001 * held;
}
