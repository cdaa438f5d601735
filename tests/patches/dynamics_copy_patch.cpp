// tests/patches/dynamics_copy_patch.cpp -- the value semantics of the drop-in maxiDynamics, plus maxiRMS and maxiRingBuf, in the
// reference's plugin form (built against include/maximilian.h only, as host/dropin_p9; tests/test_gpu_dyn_dropin.py).
// Channel 0 is a compressor in RMS mode with look-ahead.  Channel 1 is, in turn: a maxiRingBuf's tail(7) (frames < 1000), a
// maxiRMS (frames 1000 .. 2999), and from frame 3000 a COPY of the compressor made at frame 2999, fed the same input: it must
// continue with the same samples as its source.  (In the reference a copy in RMS mode keeps analysing through its source's maxiRMS --
// its detector closure holds the source's address -- so this file has no counterpart stream there.)
// The input is exact IEEE arithmetic on small integers, so the test rebuilds it.
#include "maximilian.h"

maxiDynamics comp, twin;
maxiRMS rms;
maxiRingBuf ring;
long frame = 0;

void setup() {
    comp.setAttackHigh(2);
    comp.setReleaseHigh(30);
    comp.setLookAhead(1);
    comp.setRMSWindowSize(5);
    rms.setup(100, 10);
    ring.setup(50);
}

void play(double *output) {
    const double x = ((double)((frame * 37) % 1000) / 1000.0 - 0.5) * ((frame / 700) % 2 ? 1.6 : 0.05);
    output[0] = comp.compress(x, -18, 5, 4);
    if (frame < 1000) {
        ring.push(x);
        output[1] = ring.tail(7);
    } else if (frame < 3000) {
        output[1] = rms.play(x);
        if (frame == 2999) twin = comp;
    } else {
        output[1] = twin.compress(x, -18, 5, 4);
    }
    frame++;
}
