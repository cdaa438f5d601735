// mxg_revfilt_obj.h -- one maxiReverbFilters object (reference src/libs/maxiReverb.h:42-73, .cpp:3-162; the one-pole low-pass is
// maxiFilter::lopass of src/maximilian.cpp) as plain per-sample arithmetic over a ring the caller owns.  Only + - * and compares;
// compile with contraction off.  This is the part of the step header mxg_revfilt.h that the public drop-in class of
// include/maxiReverb.h is built on, so it includes nothing but mxg_hd.h and, unlike the network part, sits in plain namespace mxg
// (inline functions, one definition in every translation unit): a class with external linkage holds an RfState.
//
// What the reference computes.  One object owns a ring of 44 100 doubles, an index, the last `size` as an int (delay_size),
// a two-point average `a`, `feedback` 0.8, `gain_cof` 0.85 and a maxiFilter whose lopass state starts at 0.  Every delay
// method stores delay_size = size (a double truncated; tapdpos takes an int), works on ring[index] and ends with
//   index != delay_size - 1 ? index++ : index = 0          (onetap compares with the DOUBLE size - 1 instead)
// so the index runs on past a size that shrank below it, and a size that grew is honoured from the next wrap on.
//   twopoint   a = 0.5 * (x + a)
//   comb1      o = ring[i];                  ring[i] = x + (feedback * o)
//   combff     o = x + ring[i];              ring[i] = x
//   combfb     o = x + (fb * ring[i]);       ring[i] = o
//   lpcombfb   y = y + (1.0 - cutoff) * (ring[i] - y);  o = x + (fb * y);  ring[i] = o
//   allpass    x += ring[i] * g;  o = ring[i] + (x * (-g));  ring[i] = x        (g = gain_cof, or the fb argument)
//   allpasstap x += ring[i] * gain_cof;  o = ring[tap slot];  ring[i] = x
//   onetap     o = ring[i];  ring[i] = x
//   tapd / tapdwgain / tapdpos: o = sum of (gain *) ring[tap slot];  ring[i] = x
//   tap slot   t = i + tap;  if (t > delay_size - 1) t -= delay_size       (gettap: the same, and nothing else)
// tapd goes through `float t = (int)(taps[k] * (size - 1)); int o = i + t;` (a float sum, truncated), tapdwgain through the
// same with the int delay_size - 1.  Where the reference would leave its 44 100 slots (an index that ran past after a shrink,
// a tapdpos position, a tap) a read gives 0.0 and a store does nothing; a double outside int's range converts as x86-64 does
// (to INT_MIN), and integer sums wrap.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

namespace mxg {

inline constexpr int RF_RING = 44100;  // slots of the reference's ring = the longest delay

// ---- the per-sample arithmetic -----------------------------------------------------------------------------------
MXG_HD double rf_twopoint(double a, double x) { return 0.5 * (x + a); }
MXG_HD double rf_comb1(double x, double feedback, double d) { return x + (feedback * d); }  // what the slot gets
MXG_HD double rf_combff(double x, double d) { return x + d; }
MXG_HD double rf_combfb(double x, double fb, double d) { return x + (fb * d); }
MXG_HD double rf_lp_coef(double cutoff) { return 1.0 - cutoff; }
MXG_HD double rf_lopass(double y, double coef, double d) { return y + coef * (d - y); }  // maxiFilter::lopass(d, coef)
// one allpass step: `t` comes in as the stage's input and leaves as its output; returns what the ring slot gets
MXG_HD double rf_allpass(double d, double g, double &t) {
    const double s = t + d * g;
    t = d + (s * (-g));
    return s;
}
// (int)x the way cvttsd2si / cvttss2si do it: out of range and NaN give INT_MIN
MXG_HD int rf_d2i(double x) { return x > -2147483649.0 && x < 2147483648.0 ? (int)x : INT32_MIN; }
MXG_HD int rf_f2i(float x) { return x >= -2147483648.0f && x < 2147483648.0f ? (int)x : INT32_MIN; }
MXG_HD int rf_add(int a, int b) { return (int)((uint32_t)a + (uint32_t)b); }
MXG_HD int rf_sub(int a, int b) { return (int)((uint32_t)a - (uint32_t)b); }

// ---- one maxiReverbFilters object over a ring of RF_RING doubles ---------------------------------------------------
struct RfState {
    double a = 0.0, output = 0.0, feedback = 0.8, gain_cof = 0.85, lp = 0.0;
    int delay_index = 0, delay_size = 0;  // (the reference leaves delay_size unset until the first call)
};
MXG_HD double rf_read(const double *ring, int i) { return (uint32_t)i < (uint32_t)RF_RING ? ring[i] : 0.0; }
MXG_HD void rf_write(double *ring, int i, double v) {
    if ((uint32_t)i < (uint32_t)RF_RING) ring[i] = v;
}
MXG_HD void rf_advance(RfState &s) { s.delay_index = s.delay_index != rf_sub(s.delay_size, 1) ? rf_add(s.delay_index, 1) : 0; }
MXG_HD int rf_tap_slot(const RfState &s, int tap) {
    int t = rf_add(s.delay_index, tap);
    if (t > rf_sub(s.delay_size, 1)) t = rf_sub(t, s.delay_size);
    return t;
}

MXG_HD double rf_obj_twopoint(RfState &s, double x) { return s.a = rf_twopoint(s.a, x); }
MXG_HD double rf_obj_comb1(RfState &s, double *ring, double x, double size) {
    s.delay_size = rf_d2i(size);
    s.output = rf_read(ring, s.delay_index);
    rf_write(ring, s.delay_index, rf_comb1(x, s.feedback, s.output));
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_combff(RfState &s, double *ring, double x, double size) {
    s.delay_size = rf_d2i(size);
    s.output = rf_combff(x, rf_read(ring, s.delay_index));
    rf_write(ring, s.delay_index, x);
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_combfb(RfState &s, double *ring, double x, double size, double fb) {
    s.delay_size = rf_d2i(size);
    s.output = rf_combfb(x, fb, rf_read(ring, s.delay_index));
    rf_write(ring, s.delay_index, s.output);
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_lpcombfb(RfState &s, double *ring, double x, double size, double fb, double cutoff) {
    s.delay_size = rf_d2i(size);
    s.lp = rf_lopass(s.lp, rf_lp_coef(cutoff), rf_read(ring, s.delay_index));
    s.output = rf_combfb(x, fb, s.lp);
    rf_write(ring, s.delay_index, s.output);
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_allpass(RfState &s, double *ring, double x, double size, double g) {
    s.delay_size = rf_d2i(size);
    rf_write(ring, s.delay_index, rf_allpass(rf_read(ring, s.delay_index), g, x));
    s.output = x;
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_allpasstap(RfState &s, double *ring, double x, double size, int tap) {
    s.delay_size = rf_d2i(size);
    x += rf_read(ring, s.delay_index) * s.gain_cof;
    s.output = rf_read(ring, rf_tap_slot(s, tap));
    rf_write(ring, s.delay_index, x);
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_gettap(RfState &s, const double *ring, int tap) { return s.output = rf_read(ring, rf_tap_slot(s, tap)); }
MXG_HD double rf_obj_onetap(RfState &s, double *ring, double x, double size) {
    s.delay_size = rf_d2i(size);
    s.output = rf_read(ring, s.delay_index);
    rf_write(ring, s.delay_index, x);
    s.delay_index = (double)s.delay_index != size - 1 ? rf_add(s.delay_index, 1) : 0;
    return s.output;
}
// the slot of tapd / tapdwgain: `scaled` = taps[k] * (size - 1), resp. taps[k] * (delay_size - 1)
MXG_HD int rf_tapd_slot(const RfState &s, double scaled) {
    const float t = (float)rf_d2i(scaled);
    int o = rf_f2i((float)s.delay_index + t);
    if (o > rf_sub(s.delay_size, 1)) o = rf_sub(o, s.delay_size);
    return o;
}
MXG_HD double rf_obj_tapd(RfState &s, double *ring, double x, double size, const double *taps, int numtaps) {
    s.output = 0.0;
    s.delay_size = rf_d2i(size);
    for (int i = 0; i < numtaps; i++) s.output += rf_read(ring, rf_tapd_slot(s, taps[i] * (size - 1)));
    rf_write(ring, s.delay_index, x);
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_tapdwgain(RfState &s, double *ring, double x, double size, const double *taps, int numtaps, const double *gain) {
    s.output = 0.0;
    s.delay_size = rf_d2i(size);
    for (int i = 0; i < numtaps; i++) s.output += gain[i] * rf_read(ring, rf_tapd_slot(s, taps[i] * rf_sub(s.delay_size, 1)));
    rf_write(ring, s.delay_index, x);
    rf_advance(s);
    return s.output;
}
MXG_HD double rf_obj_tapdpos(RfState &s, double *ring, double x, int size, const int *taps, int numtaps) {
    s.output = 0.0;
    s.delay_size = size;
    for (int i = 0; i < numtaps; i++) s.output += rf_read(ring, taps[i]);
    rf_write(ring, s.delay_index, x);
    rf_advance(s);
    return s.output;
}

}  // namespace mxg
