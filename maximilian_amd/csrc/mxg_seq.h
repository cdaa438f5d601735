// mxg_seq.h -- the reference's sequencing helpers as plain per-sample arithmetic over small state structs: maxiTrigger::onZX
// (H:569-579), maxiRatioSeq::playTrig / playValues (H:2165-2223), maxiStep::pull (H:2103-2130), maxiCounter::count (H:1961-1972),
// maxiIndex::pull (H:1992-2008) and maxiZXToPulse::play (H:2245-2258).  H = src/maximilian.h.  No device state: the same text
// compiles for the host (tests/host_seq.cpp, the checker of the GPU tests).  Everything is compares, + - / floor and integer
// indexing: bit-exact, no tolerance anywhere.
//
// What is reproduced is what the reference computes:
//   * playTrig's first call sets prevPhase = phase - 1/sampleRate; a wrap (prevPhase > phase) sets prevPhase = -1/sampleRate;
//   * the boundaries are acc_i / sum accumulated left to right, a boundary equal to 1.0 becomes 0.0 (mxg_seq_ratio_host builds
//     that table once per pattern, with the reference's operations in the reference's order); the trigger is the OR over the
//     boundaries of prev <= b && phase > b, so a zero or NaN sum (boundaries inf / NaN) never fires;
//   * playValues: a change of the value list's length sets counter = len - 1 BEFORE the trigger is looked at;
//   * maxiStep: the first trigger sets index = 0 without stepping, step > len is clamped to len, index is a double and the
//     value read is values[(size_t)index] on EVERY sample;
//   * maxiStep / maxiIndex / maxiCounter / maxiZXToPulse look at their trigger through a maxiTrigger of their own: two
//     consecutive 1s fire once; maxiCounter increments before it resets; maxiIndex reads floor(idx * 0.99999999 * len) after
//     clamping idx to [0, 1].
// The one departure: a read index is held inside its table (seq_hold) where the reference would index out of bounds --
// maxiStep with step < -len (index stays negative), a NaN index, a carried state that was uploaded out of range.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mxg_hd.h"
#include "mxg_osc.h"  // the clock: maxiOsc::phasor's increment and recurrence

namespace mxg {
namespace {

struct SeqZx {  // maxiTrigger (H:593-595: previousValue = 1, firstTrigger = 1)
    double prev;
    bool first;
};
struct SeqRatio {  // maxiRatioSeq (H:2226-2229)
    double prevPhase;
    bool first;
    long long counter, lengthOfValues;
};
struct SeqStep {  // maxiStep (H:2138-2140)
    SeqZx trig;
    bool first;
    double index;
};
struct SeqCounter {  // maxiCounter (H:1975-1976)
    double value;
    SeqZx inc, rst;
};
struct SeqIndex {  // maxiIndex (H:2011-2012)
    SeqZx trig;
    double value;
};
struct SeqPulse {  // maxiZXToPulse (H:2260-2261)
    SeqZx trig;
    double hold;
};

// a read index held inside a table of len >= 1 entries (the departure above; NaN -> 0)
MXG_HD int seq_hold(double index, int len) {
    if (!(index >= 1.0)) return 0;
    if (index >= (double)len) return len - 1;
    return (int)index;
}
MXG_HD int seq_hold(long long index, int len) { return index < 0 ? 0 : (index >= len ? len - 1 : (int)index); }

MXG_HD double seq_onzx(SeqZx &z, double input) {  // H:569-579
    const bool zx = (z.prev <= 0.0 || z.first) && input > 0;
    z.prev = input;
    z.first = false;
    return zx ? 1.0 : 0.0;
}

// playTrig H:2165-2195 against the boundary table of the pattern (bounds[i] = acc_i / sum, 1.0 -> 0.0); inv_sr = 1.0 / sampleRate
MXG_HD double seq_ratio_trig(SeqRatio &r, double phase, const double *bounds, int len, double inv_sr) {
    if (r.first) {
        r.first = false;
        r.prevPhase = phase - inv_sr;
    }
    if (r.prevPhase > phase) r.prevPhase = -inv_sr;  // the wrapping point
    bool trig = false;
    for (int i = 0; i < len; i++) {
        const double b = bounds[i];
        trig = trig || (r.prevPhase <= b && phase > b);
    }
    r.prevPhase = phase;
    return trig ? 1.0 : 0.0;
}

// playValues H:2204-2223; *trig_out (optional) receives playTrig's result
MXG_HD double seq_ratio_values(SeqRatio &r, double phase, const double *bounds, int len, double inv_sr, const double *values,
                               int vallen, double *trig_out) {
    if (r.lengthOfValues != vallen) {
        r.lengthOfValues = vallen;
        r.counter = (long long)vallen - 1;
    }
    const double t = seq_ratio_trig(r, phase, bounds, len, inv_sr);
    if (t != 0.0) {
        r.counter++;
        if (r.counter == vallen) r.counter = 0;
    }
    if (trig_out) *trig_out = t;
    return values[seq_hold(r.counter, vallen)];
}

MXG_HD double seq_step_pull(SeqStep &s, double trigSig, const double *values, int len, double step) {  // H:2103-2130
    if (seq_onzx(s.trig, trigSig) != 0.0) {
        if (s.first) {
            s.first = false;
            s.index = 0;
        } else {
            const double arrayLen = (double)len;
            if (step > arrayLen) step = arrayLen;
            s.index = s.index + step;
            if (s.index < 0) s.index = arrayLen + s.index;
            else if (s.index >= arrayLen) s.index = s.index - arrayLen;
        }
    }
    return values[seq_hold(s.index, len)];
}

MXG_HD double seq_counter(SeqCounter &c, double incTrigger, double resetTrigger) {  // H:1961-1972
    if (seq_onzx(c.inc, incTrigger) != 0.0) c.value = c.value + 1;
    if (seq_onzx(c.rst, resetTrigger) != 0.0) c.value = 0;
    return c.value;
}

MXG_HD double seq_index_pull(SeqIndex &x, double trigSig, double indexSig, const double *values, int len) {  // H:1992-2008
    if (seq_onzx(x.trig, trigSig) != 0.0) {
        if (indexSig < 0) indexSig = 0;
        if (indexSig > 1) indexSig = 1;
        x.value = values[seq_hold(floor(indexSig * 0.99999999 * (double)len), len)];
    }
    return x.value;
}

MXG_HD double seq_pulse(SeqPulse &p, double input, double holdTimeInSamples) {  // H:2245-2258
    double output = 0;
    if (seq_onzx(p.trig, input) != 0.0) p.hold = holdTimeInSamples;
    if (p.hold > 0) {
        output = 1;
        p.hold = p.hold - 1;
    }
    return output;
}

// One pattern's boundary table, the reference's operations in the reference's order (H:2172-2186); entries past len never fire.
MXG_HD void seq_ratio_bounds(const double *times, int len, int L, double *norm) {
    double sum = 0;
    for (int i = 0; i < len; i++) sum += times[i];
    double accumulatedTime = 0;
    for (int i = 0; i < L; i++) {
        if (i >= len) {
            norm[i] = NAN;
            continue;
        }
        accumulatedTime += times[i];
        double normalisedTime = accumulatedTime / sum;
        if (normalisedTime == 1.0) normalisedTime = 0.0;
        norm[i] = normalisedTime;
    }
}

// ---- the fused sequencer: clock -> playTrig -> playValues | maxiStep::pull -> maxiZXToPulse::play ---------------------------------
// Which stages run (a stage whose output is not wanted does not run and its state is untouched; playTrig always runs).
#define MXG_SEQ_WANT_VALUES 1  // the value output is playValues
#define MXG_SEQ_WANT_STEP 2    // the value output is maxiStep::pull(trig, values, step)
#define MXG_SEQ_WANT_GATE 4    // maxiZXToPulse::play(trig, hold)

struct SeqVoiceCfg {
    const double *bounds;  // the voice's pattern
    int len;
    const double *values;  // the voice's value list
    int vlen;
    double step, hold, inv_sr;
    int want;
};

MXG_HD void seq_voice_tick(SeqRatio &r, SeqStep &st, SeqPulse &pu, const SeqVoiceCfg &c, double phase, double &trig, double &val,
                           double &gate) {
    if (c.want & MXG_SEQ_WANT_VALUES) {
        val = seq_ratio_values(r, phase, c.bounds, c.len, c.inv_sr, c.values, c.vlen, &trig);
    } else {
        trig = seq_ratio_trig(r, phase, c.bounds, c.len, c.inv_sr);
        if (c.want & MXG_SEQ_WANT_STEP) val = seq_step_pull(st, trig, c.values, c.vlen, c.step);
    }
    if (c.want & MXG_SEQ_WANT_GATE) gate = seq_pulse(pu, trig, c.hold);
}

// the internal clock: maxiOsc::phasor(freq) (C:285-291), mxg_osc.h's increment and recurrence
MXG_HD double seq_clock_tick(double &clk, const OscPre &q) {
    double hold;
    return osc_tick<MXG_OSC_PHASOR>(clk, hold, q, nullptr, nullptr);
}

}  // namespace
}  // namespace mxg
