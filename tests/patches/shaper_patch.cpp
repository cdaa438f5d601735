// tests/patches/shaper_patch.cpp -- a patch in the reference's plugin form that touches every member of maxiNonlinearity (through
// the maxiDistortion alias too), maxiXFade (both overloads), maxiSelect, maxiSelectX, maxiLine (prepare / triggerEnable /
// isLineComplete / play) and maxiBits (every static member but noise(); widths stay <= 31).  The sources are maxiOsc::saw,
// phasor and triangle only, which are exact on the device, so output[0] -- hardclip, fastatan, fastAtanDist, the cross-fades,
// the selects, the lines and the bit signals -- is the reference's bits (tests/test_gpu_shaper_dropin.py;
// tests/golden/shaper.npz["patch"]).  output[1] carries what goes through the host libm: softclip (pow), atanDist and asymclip.
// Built against include/maximilian.h as host/dropin_sh.  With -DSHAPER_PATCH_ARITH the three sources are plain arithmetic
// instead of oscillators, and the patch runs without a device (tests/test_shaper_dropin_cpu.py).
#include "maximilian.h"

#ifdef SHAPER_PATCH_ARITH
struct ArithOsc {  // a ramp of the given rate per sample, in [0, 1)
    double ph = 0;
    double phasor(double f) { ph += f / 44100.0; if (ph >= 1.0) ph -= 1.0; return ph; }
    double saw(double f) { return 2.0 * phasor(f) - 1.0; }
    double triangle(double f) { const double p = phasor(f); return p < 0.5 ? 4.0 * p - 1.0 : 3.0 - 4.0 * p; }
};
typedef ArithOsc Source;
#else
typedef maxiOsc Source;
#endif

Source o1, o2, lfo, clk;
maxiDistortion dist;
maxiNonlinearity nl;
maxiXFade xf;
maxiSelect sel;
maxiSelectX selx;
maxiLine line, loop, gated;
std::vector<double> vals = {0.25, -0.5, 1.0, 0.125};
long frame = 0;
int rests = 0;

void setup() {
    line.prepare(0.0, 1.0, 10.0, true);
    line.triggerEnable(1);
    loop.prepare(1.0, -1.0, 4.0, false);
    loop.triggerEnable(0.5);
    gated.prepare(0.5, 2.0, 3.0, false);  // stays disabled until frame 1500
    gated.triggerEnable(-1);
}

void play(double *output) {
    typedef maxiBits::bitsig bitsig;
    const double s = o1.saw(110) * 1.4;  // past +-1: the clipped branches
    const double t = o2.triangle(57.3) * 1.2;
    const double ph = lfo.phasor(3.1);
    const double trig = clk.phasor(40) - 0.5;
    const double ln = line.play(trig), lp = loop.play(trig), gt = gated.play(trig);
    if (line.isLineComplete() && ++rests == 300) {  // a one-shot line re-arms only when it is prepared again
        line.prepare(0.25, 0.75, 6.0, true);
        rests = 0;
    }
    if (frame == 1500) gated.triggerEnable(1);
    const double shaped = dist.hardclip(s) + nl.fastatan(t) + dist.fastAtanDist(t, 3.0) + nl.hardclip(t);
    const double mono = maxiXFade::xfade(s, t, lp * 1.2);
    std::vector<double> c1 = {s, ln}, c2 = {t, gt};
    const std::vector<double> st = xf.xfade(c1, c2, 2.0 * ph - 1.0);
    std::vector<double> sig = {s, t, ln, lp};
    const double picked = sel.play(ph, vals, true) + selx.play(ph * 4.5 - 0.25, vals, false) + 0.5 * selx.play(ph * 1.1 - 0.05, sig, true) +
                          0.25 * sel.play(ph * 5.0 - 0.5, sig, false);
    const bitsig b = maxiBits::fromSignal(2.0 * ph - 1.0), c = maxiBits::sig((bitsig)frame);
    bitsig y = maxiBits::lxor(maxiBits::land(b, maxiBits::shr(b, 7)), maxiBits::lor(c, maxiBits::shl(maxiBits::l(5), 3)));
    y = maxiBits::add(y, maxiBits::mul(maxiBits::inc(c), 2654435761u));
    y = maxiBits::neg(maxiBits::sub(y, maxiBits::dec(b)));
    y = maxiBits::div(y, maxiBits::lor(maxiBits::r(c, 9, 4), 1));
    const bitsig flags = maxiBits::gt(b, c) + 2 * maxiBits::lt(b, c) + 4 * maxiBits::gte(b, y) + 8 * maxiBits::lte(b, y) +
                         16 * maxiBits::eq(maxiBits::at(c, 3), 1) + 32 * maxiBits::ct(y, 31);
    const double bits = 0.25 * maxiBits::toSignal(y) + 0.125 * maxiBits::toTrigSignal(maxiBits::at(c, 10)) + (double)flags / 4096.0;
    output[0] = 0.25 * shaped + 0.5 * mono + 0.25 * (st[0] + st[1]) + 0.125 * picked + 0.25 * bits;
    output[1] = nl.softclip(t) + dist.atanDist(s, 4.0) + 0.5 * nl.asymclip(t, 0.7, 2.5);
    frame++;
}
