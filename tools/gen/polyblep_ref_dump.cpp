// tools/gen/polyblep_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiPolyBLEP: tools/gen/gen_golden_polyblep.py compiles it, together with the UNMODIFIED reference sources, into a shared
// library in a temporary directory and drives it block by block to write tests/golden/polyblep.npz.
//
// V maxiPolyBLEP objects live side by side and are called sample-major; the phase is read through -fno-access-control.
#include <cstdint>
#include <vector>

#include "maximilian.h"
#include "libs/maxiPolyBLEP.h"

typedef std::vector<maxiPolyBLEP> Bank;

extern "C" {

void pb_set_rate(int sr) { maxiSettings::sampleRate = sr; }

void *pb_new(size_t V) { return new Bank(V); }
void pb_free(void *h) { delete (Bank *)h; }

void pb_waveform(void *h, int wf) {
    for (auto &o : *(Bank *)h) o.setWaveform((maxiPolyBLEP::Waveform)wf);
}
void pb_pulse_width(void *h, size_t v, double pw) { (*(Bank *)h)[v].setPulseWidth(pw); }
void pb_sync(void *h, size_t v, double phase) { (*(Bank *)h)[v].sync(phase); }

// freq, out [n][V]
void pb_play(void *h, size_t n, const double *freq, double *out) {
    Bank &b = *(Bank *)h;
    const size_t V = b.size();
    for (size_t i = 0; i < n; i++)
        for (size_t v = 0; v < V; v++) out[i * V + v] = b[v].play(freq[i * V + v]);
}

void pb_phase(void *h, double *t) {
    Bank &b = *(Bank *)h;
    for (size_t v = 0; v < b.size(); v++) t[v] = b[v].blep.t;
}

// the enum's values, in the order the names are listed in tests/polyblep_host.py
void pb_enum(int *out) {
    typedef maxiPolyBLEP::Waveform W;
    const W all[14] = {W::SINE, W::COSINE, W::TRIANGLE, W::SQUARE, W::RECTANGLE, W::SAWTOOTH, W::RAMP, W::MODIFIED_TRIANGLE,
                       W::MODIFIED_SQUARE, W::HALF_WAVE_RECTIFIED_SINE, W::FULL_WAVE_RECTIFIED_SINE, W::TRIANGULAR_PULSE,
                       W::TRAPEZOID_FIXED, W::TRAPEZOID_VARIABLE};
    for (int i = 0; i < 14; i++) out[i] = (int)all[i];
}

// A maxiEnvGen after setup(levels, times, curves, false): the edits ops [nops][3] = (kind: 0 setLevel, 1 setCurve; index; value) one
// after the other.  out [nops][nstages][6]: the stage table after each edit in include/maxigpu.h's layout (startlevel, endlevel,
// gradient, curve, length, hold); ret [nops]: what the call returned.
void pb_envgen_edits(size_t nlevels, const double *levels, const double *times, const double *curves, size_t nops, const double *ops,
                     double *out, int *ret) {
    maxiEnvGen e;
    e.setup(std::vector<double>(levels, levels + nlevels), std::vector<double>(times, times + nlevels - 1),
            std::vector<double>(curves, curves + nlevels - 1), false);
    const size_t ns = e.stages.size();
    for (size_t i = 0; i < nops; i++) {
        const size_t index = (size_t)ops[3 * i + 1];
        ret[i] = ops[3 * i] == 0 ? e.setLevel(index, ops[3 * i + 2]) : e.setCurve(index, ops[3 * i + 2]);
        for (size_t k = 0; k < ns; k++) {
            double *row = out + (i * ns + k) * 6;
            row[0] = e.stages[k].startlevel; row[1] = e.stages[k].endlevel; row[2] = e.stages[k].gradient;
            row[3] = e.stages[k].curve; row[4] = (double)e.stages[k].length; row[5] = e.stages[k].hold ? 1.0 : 0.0;
        }
    }
}

}  // extern "C"
