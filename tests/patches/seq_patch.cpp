// tests/patches/seq_patch.cpp -- a sequenced voice in the reference's plugin form, after the graph of the reference's example
// 9.Envelopes3: a clock phasor whose rate is moved by a slow envelope drives maxiRatioSeq::playTrig, the trigger plays an
// amplitude envelope and pulls the pitch from a list with maxiStep; two detuned oscillators go through a maxiSVF whose cutoff
// a third envelope moves.  maxiOsc::saw stands where the example has maxiPolyBLEP, and the envelopes have curve 1 and a fixed
// shape.  A maxiCounter (reset by a slow saw), a maxiIndex (read position from a triangle LFO) and a maxiZXToPulse colour the
// level.  Channel 1 is a second voice on a fixed clock, envelope * oscillator and nothing else: the form a bank renders
// (tests/test_gpu_seq.py chains mxg_seq_render -> mxg_envgen_render -> mxg_osc_render and compares its voice 0 with it).
// Built against include/maximilian.h as host/dropin_sq (tests/test_gpu_seq_dropin.py) and, for tests/golden/seq.npz["patch"],
// against the reference sources by tools/gen/gen_golden_seq.py.
#include "maximilian.h"

maxiOsc osc1, osc2, clockPhase, resetSaw, indexLfo, clockB, oscB;
maxiEnvGen ampEnv, ctlEnv, cutEnv, envB;
maxiSVF filter;
maxiRatioSeq rseq, rseqB;
maxiStep pitchStep, stepB;
maxiCounter counter;
maxiIndex picker;
maxiZXToPulse pulse;
std::vector<double> levels = {0.25, 0.5, 1.0, 0.75};

void setup() {
    ampEnv.setup({0, 1, 0.2, 0}, {5, 4, 2}, {1, 1, 1}, false, true);
    ctlEnv.setup({0.1, 1}, {250}, {1}, false);
    cutEnv.setup({100, 200}, {250}, {1}, false);
    envB.setup({0, 1, 0.2, 0}, {5, 4, 2}, {1, 1, 1}, false, true);
    filter.setResonance(0.2);
}

void play(double *output) {
    const double controller = ctlEnv.play(1);
    const double cl = clockPhase.phasor(90 - (controller * 60));
    const double trig = rseq.playTrig(cl, {3, 3, 2});
    const double ampenv = ampEnv.play(trig);
    const double frequency = pitchStep.pull(trig, {40, 80, 170, 350, 900, 3888}, 1);
    double w = osc1.saw(frequency) + osc2.saw(frequency * (1.02 + (controller * 0.13)));
    w = w * ampenv;
    const double hits = counter.count(trig, resetSaw.phasor(11) - 0.5);
    const double level = picker.pull(trig, indexLfo.triangle(7) * 0.6 + 0.5, levels);
    w = w * (0.5 + 0.05 * hits) * (0.25 + level) + 0.01 * pulse.play(trig, 120);
    filter.setCutoff(cutEnv.play(1));
    w = filter.play(w, 0, 1, 0.3, 0);
    output[0] = w;
    const double trigB = rseqB.playTrig(clockB.phasor(47), {4, 4, 4, 1, 1, 1, 1});
    const double freqB = stepB.pull(trigB, {40, 80, 170, 350, 900, 3888}, 1);
    output[1] = envB.play(trigB) * oscB.saw(freqB);
}
