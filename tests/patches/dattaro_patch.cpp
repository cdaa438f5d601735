// tests/patches/dattaro_patch.cpp -- maxiDattaroReverb behind an enveloped oscillator: one object constructed at 44 100 Hz and
// one at 22 050 Hz (the constructor fixes the delay lengths from maxiSettings::sampleRate; the rate is put back afterwards and the
// second object keeps its lengths), a copy made mid-stream and played beside its source, and an object that is destroyed and
// constructed again mid-stream (silent rings again).  The objects that are not statics are constructed in zeroed static storage,
// as statics are: the reference's maxiFilter leaves its state unset.
// Built against include/ as host/dropin_dt (tests/test_gpu_dattaro_dropin.py) and, for tests/golden/dattaro.npz["patch"], against
// the reference sources by tools/gen/gen_golden_dattaro.py.
#include <cstring>
#include <new>

#include "maximilian.h"
#include "maxiReverb.h"

maxiOsc osc;
maxiEnv env;
maxiDattaroReverb plate, plateCopy;
alignas(maxiDattaroReverb) static unsigned char halfMem[sizeof(maxiDattaroReverb)], againMem[sizeof(maxiDattaroReverb)];
maxiDattaroReverb *half = nullptr, *again = nullptr;
long frame = 0;

void setup() {
    env.setAttack(5);
    env.setDecay(50);
    env.setSustain(0.4);
    env.setRelease(300);
    maxiSettings::setup(22050, 2, 512);
    half = new (halfMem) maxiDattaroReverb;
    maxiSettings::setup(44100, 2, 512);
    again = new (againMem) maxiDattaroReverb;
}

void play(double *output) {
    const int trig = (frame % 1500) < 200;
    const double w = osc.saw(110) * env.adsr(0.5, trig);
    double *a = plate.playStereo(w);
    double l = a[0], r = a[1];
    double *b = half->playStereo(w * 0.5);
    l += b[0];
    r += b[1];
    if (frame == 2600) plateCopy = plate;
    if (frame == 3100) {
        again->~maxiDattaroReverb();
        std::memset(againMem, 0, sizeof(againMem));
        again = new (againMem) maxiDattaroReverb;
    }
    double *c = again->playStereo(-w);
    l += c[0] * 0.25;
    r += c[1] * 0.25;
    if (frame >= 2600) {
        double *d = plateCopy.playStereo(w);  // = a
        l -= d[1];
        r -= d[0];
    }
    output[0] = l;
    output[1] = r;
    frame++;
}
