// tests/patches/revfilt_patch.cpp -- every public method of maxiReverbFilters on objects of their own, 16 output channels, fed by
// an integer noise source (no oscillator: the patch needs no device).  Sizes 1, 2 and 44 100, non-integer sizes, a size that
// grows mid-stream, one that shrinks below the index for fewer samples than the ring has left, onetap's never-wrapping compare
// at a non-integer size, tapd / tapdwgain with taps 0.0 and 1.0, tapdpos at both ends of the ring, gettap after each kind of
// call, and copies (an assignment and a std::vector that reallocates) that continue apart from their sources.
// Built against include/ by tests/test_revfilt_dropin_cpu.py and, for tests/golden/revnet.npz["patch"], against the reference
// sources by tools/gen/gen_golden_revnet.py.  The objects are static: zero-initialised before their constructors run, which the
// reference needs (maxiFilter's constructor leaves its state unset).
#include <cstdint>
#include <vector>

#include "maximilian.h"
#include "maxiReverb.h"

static maxiReverbFilters tp, c1, cff, cfbBig, cfb2, lpc, lpc64, apGrow, apShrink, apTap, ap1, ap2, one, oneFrac, td, tg, tpos, lpcCopy;
static std::vector<maxiReverbFilters> vec;
static uint64_t seed = 0x9e3779b97f4a7c15ull;
static long frame = 0;

static double noise() {  // uniform in [-1, 1): integer arithmetic and one exact scaling
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(seed >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

void setup() {
    maxiSettings::setup(44100, 16, 1024);
    vec.resize(1);
}

void play(double *output) {
    double x = noise();
    if (frame >= 1800) x = 0.0;  // the tail
    static double taps[4] = {0.0, 1.0, 0.5, 0.123};
    static double gains[3] = {0.5, -0.25, 1.5};
    static int pos[4] = {0, 299, 17, 44099};

    // (one call per statement: the operands of a + are not sequenced)
    double o[16];
    o[0] = tp.twopoint(x);
    o[0] += tp.gettap(0);
    o[1] = c1.comb1(x, 1);
    o[1] += c1.gettap(0);
    o[2] = cff.combff(x, 2);
    o[2] += cff.gettap(1);
    o[3] = cfbBig.combfb(x, 44100, 0.7);
    o[3] += cfbBig.gettap(44099);
    o[4] = lpc.lpcombfb(x, 347.6, 0.84, 0.2);
    o[4] += lpc.gettap(5);
    o[5] = apGrow.allpass(x, frame < 1000 ? 100 : 250);
    o[5] += apGrow.gettap(3);
    // 300 until the index stands at 100, then 50 for 400 samples (the index runs on to 500), then 600
    o[6] = apShrink.allpass(x, frame < 1000 ? 300 : frame < 1400 ? 50 : 600, -0.6);
    o[6] += apShrink.gettap(7);
    o[7] = apTap.allpasstap(x, 200, 37);
    o[7] += apTap.gettap(199);
    o[8] = one.onetap(x, 10);
    o[8] += one.gettap(2);
    o[8] += oneFrac.onetap(x, 64.5);
    o[8] += oneFrac.gettap(1);
    o[9] = td.tapd(x, 500, taps, 4);
    o[9] += td.gettap(11);
    o[10] = tg.tapdwgain(x, 321.7, taps + 1, 3, gains);
    o[10] += tg.tapdwgain(-x, 321.7, taps, 1, gains + 2);
    o[10] += tg.gettap(0);
    o[11] = tpos.tapdpos(x, 300, pos, 4);
    o[11] += tpos.gettap(299);
    if (frame == 1200) {
        lpcCopy = lpc;
        vec.push_back(apGrow);  // a copy, and a reallocation that copies the other element
    }
    o[12] = frame >= 1200 ? lpcCopy.lpcombfb(-x, 347.6, 0.84, 0.2) : 0.0;
    o[13] = vec[0].combfb(x, 77, -0.5);
    if (frame >= 1200) o[13] += vec[1].allpass(x * 0.5, 250);
    o[14] = ap1.allpass(x, 1, 0.5);
    o[14] += ap2.allpass(x, 2);
    o[15] = cfb2.combfb(x, 2, 0.9);
    o[15] += lpc64.lpcombfb(x, 64, 1.02, -0.1);
    o[15] += lpc64.gettap(63);
    for (int k = 0; k < 16; k++) output[k] = o[k];
    frame++;
}
