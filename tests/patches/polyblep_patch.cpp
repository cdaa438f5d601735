// tests/patches/polyblep_patch.cpp -- a patch in the reference's plugin form around maxiPolyBLEP.  output[0] sums the ten waveforms
// that are plain arithmetic -- TRIANGLE, SQUARE, RECTANGLE, SAWTOOTH, RAMP, MODIFIED_TRIANGLE, MODIFIED_SQUARE, TRIANGULAR_PULSE,
// TRAPEZOID_FIXED, TRAPEZOID_VARIABLE -- with frequencies and pulse widths driven by sources that are exact on the device
// (maxiOsc::phasor, saw and triangle, and a maxiEnvGen of curve 1 whose levels move with setLevel), all well below
// sampleRate / 4, plus a sync() in mid-run, a setPulseWidth in mid-run, a setSampleRate and a copied object: it is the
// reference's bits (tests/test_gpu_polyblep_dropin.py; tests/golden/polyblep.npz["patch"]).  output[1] sums the four sine
// waveforms and a sawtooth that is swept through sampleRate / 4, where it becomes a sine: within the sum of their bounds.
// Built against include/maximilian.h as host/dropin_pb.
#include "maximilian.h"
#include "libs/maxiPolyBLEP.h"

typedef maxiPolyBLEP::Waveform W;
const W kExact[10] = {W::TRIANGLE, W::SQUARE, W::RECTANGLE, W::SAWTOOTH, W::RAMP, W::MODIFIED_TRIANGLE, W::MODIFIED_SQUARE,
                      W::TRIANGULAR_PULSE, W::TRAPEZOID_FIXED, W::TRAPEZOID_VARIABLE};
const W kSine[4] = {W::SINE, W::COSINE, W::HALF_WAVE_RECTIFIED_SINE, W::FULL_WAVE_RECTIFIED_SINE};

maxiPolyBLEP exact[10], sine[4], sweep, twin, back;
maxiOsc lfo1, lfo2, lfo3;
maxiEnvGen env;
long frame = 0;

void setup() {
    for (int i = 0; i < 10; i++) {
        exact[i].setWaveform(kExact[i]);
        exact[i].setPulseWidth(0.1 + 0.08 * i);
    }
    for (int i = 0; i < 4; i++) sine[i].setWaveform(kSine[i]);
    sweep.setWaveform(W::SAWTOOTH);
    twin.setWaveform(W::SQUARE);
    back.setWaveform(W::RAMP);
    env.setup({0, 1, 0.25, 0}, {5, 8, 11}, {1, 1, 1}, true);
}

void play(double *output) {
    const double tri = lfo1.triangle(3.7), saw = lfo2.saw(0.9), ph = lfo3.phasor(11.0);
    const double e = env.play(frame % 1500 < 900 ? 1.0 : -1.0);  // (a plain gate: the engine predicts whole blocks of it)
    if (frame % 512 == 100) {  // the levels of the running envelope move: startlevel of stage 1 with endlevel of stage 0, the last endlevel
        env.setLevel(1, 0.5 + 0.25 * (double)((frame / 512) % 3));
        env.setLevel(3, 0.125 * (double)((frame / 512) % 2));
        env.setCurve(3, 7.0);  // (outside the table: nothing)
    }
    if (frame == 2048) {  // on a block edge of the per-sample engine, and once more two samples later
        exact[3].sync(2.75);
        exact[0].sync(-0.25);
    }
    if (frame == 2050) exact[6].sync(-3.0);
    if (frame == 3000) {
        exact[2].setPulseWidth(0.99995);
        exact[5].setPulseWidth(0.00005);
        exact[9].setPulseWidth(1.0);
        exact[7].setPulseWidth(0.0);
    }
    if (frame == 3500) exact[7].setPulseWidth(0.625);
    if (frame == 1000) twin = exact[1];  // a copy continues from the same phase
    if (frame == 4000) exact[4].setSampleRate(48000);
    double a = 0;
    for (int i = 0; i < 10; i++) {
        const double base = 55.0 * (double)(i + 1);  // (one source per frequency: a form the per-sample engine predicts in blocks)
        const double f = i % 4 == 0 ? base + 100.0 * e : (i % 4 == 1 ? base + 40.0 * tri : (i % 4 == 2 ? base + 30.0 * saw : base + 25.0 * ph));
        a += exact[i].play(f);
    }
    a += twin.play(220.0 + 40.0 * tri) + back.play(-330.0 - 20.0 * ph);  // (a negative frequency runs the phase backwards)
    output[0] = a / 12.0;
    double b = 0;
    for (int i = 0; i < 4; i++) b += sine[i].play(110.0 * (double)(i + 1) + 20.0 * saw);
    b += sweep.play(11025.0 + 6000.0 * tri);
    output[1] = b / 5.0;
    frame++;
}
