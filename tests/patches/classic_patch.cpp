// tests/patches/classic_patch.cpp -- a patch in the reference's plugin form around the classic core classes: maxiOsc::saw / phasor
// sources (exact on the device; no sinewave), gated and compressed by maxiDyn objects, shaped by a maxiEnvelope that is triggered
// again while it runs, smoothed by a maxiLagExp, ranges through maxiMap::linlin and clamp.  output[0] carries what is plain
// arithmetic -- the gate, the envelope, the lag, the maps -- and is the reference's bits (tests/golden/classic.npz["patch"]);
// output[1] carries the compressors, whose make-up factor (log) and setter coefficients (pow) go through the host libm.
// Built against include/maximilian.h as host/dropin_cl.  With -DCLASSIC_PATCH_ARITH the sources are plain arithmetic instead of
// oscillators, and the patch runs without a device (tests/test_classic_dropin_cpu.py; classic.npz["patch_arith"]).
#include "maximilian.h"

#ifdef CLASSIC_PATCH_ARITH
struct ArithOsc {  // a ramp of the given rate per sample, in [0, 1)
    double ph = 0;
    double phasor(double f) { ph += f / 44100.0; if (ph >= 1.0) ph -= 1.0; return ph; }
    double saw(double f) { return 2.0 * phasor(f) - 1.0; }
};
typedef ArithOsc Source;
#else
typedef maxiOsc Source;
#endif

Source o1, o2, lfo, clk;
maxiDyn gate, comp, comp2;
maxiEnvelope env;
maxiLagExp<double> lag(0.05, 0.0);
std::vector<double> segs = {1.0, 2.0, 0.3, 4.0, 0.8, 1.0, 0.0, 3.0};
long frame = 0;

void setup() {
    comp2.setRatio(3.0);
    comp2.setThreshold(0.4);
    comp2.setAttack(2.0);
    comp2.setRelease(1.5);
}

void play(double *output) {
    const double s = o1.saw(110) * 1.2;
    const double ph = lfo.phasor(2.5);
    const double t = clk.phasor(5.0);
    const double am = maxiMap::linlin(ph, 0.2, 0.8, 0.0, 1.0);  // passes both clips
    const double sig = s * am;
    if (frame % 1500 == 0) env.trigger(0, 0.01);  // the second trigger arrives in the middle of a segment
    const double e = env.line(8, segs);
    const double g = gate.gate(sig, 0.5, 30, 0.2, 0.999);
    lag.addSample(t < 0.5 ? 1.0 : -0.25);
    const double cutoff = maxiMap::linlin(lag.value(), -0.25, 1.0, 100.0, 4000.0);
    output[0] = 0.5 * g + 0.25 * e * sig + cutoff / 16000.0 + 0.125 * maxiMap::clamp(s, -0.5, 0.75);
    output[1] = 0.5 * comp.compressor(sig, 4.0, 0.5, 0.3, 0.99) + 0.5 * comp2.compress(o2.saw(57.3));
    frame++;
}
