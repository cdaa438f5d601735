// mxg_fx.h -- maxiFlanger (H:1166-1172) and maxiChorus (H:1202-1212) as plain per-sample arithmetic, plus the
// tap-size / ring-phase trajectory and the time-tile classifier that fx.hip's kernels are built on.
// No device state and only + - * / compares and conversions: the same text compiles for the host, which is how
// tests/test_fx_host.py fuzzes the trajectory and the tile classification (tests/host_fx.cpp).
//
// Reference (C = src/maximilian.cpp, H = src/maximilian.h):
//   maxiOsc::triangle C:362-373   phase wraps by -1 BEFORE the step, inc = 1./(sr/speed)
//   maxiOsc::noise    C:214-220   float r = rand()/(float)RAND_MAX; output = r*2-1 (float arithmetic)
//   maxiFilter::lores C:455-468   the (c, r) pair comes from the host libm (mxg_filter_coeffs_host)
//   maxiDelayline::dl C:420-429   if (phase >= size) phase = 0; out = mem[phase]; mem[phase] = mem*fb + (in*fb)*0.5
#pragma once
#include <math.h>
#include <stdint.h>

#include "mxg_hd.h"

namespace mxg {
namespace {

// ---- double -> int as x86-64 converts it (cvttsd2si) --------------------------------------------
// The reference passes a double to dl's `int size`.  x86 truncates toward zero and yields INT_MIN
// (0x80000000, "integer indefinite") for NaN and for anything outside (-2^31-1, 2^31);
// v_cvt_i32_f64 would saturate instead, and C++ calls it undefined, so the range is tested here.
MXG_HD int fx_cvt_i32(double d) {
    return (d > -2147483649.0 && d < 2147483648.0) ? (int)d : (-2147483647 - 1);
}

// ---- the LFOs ------------------------------------------------------------------------------------
MXG_HD double fx_tri_inc(double sr, double speed) { return 1. / (sr / speed); }  // C:364 (sr = (double)size_t)

MXG_HD double fx_triangle(double &phase, double inc) {  // C:362-373
    if (phase >= 1.0) phase -= 1.0;
    phase += inc;
    return phase <= 0.5 ? (phase - 0.25) * 4 : ((1.0 - phase) - 0.25) * 4;
}

MXG_HD double fx_noise(int32_t rnd) {  // C:214-220: (float)RAND_MAX = 2^31 exactly, the arithmetic is float
    const float r = (float)rnd / 2147483648.0f;
    return (double)(r * 2.0f - 1.0f);
}

MXG_HD double fx_lores(double &x, double &y, double input, double c, double r) {  // C:463-467
    x = x + (input - y) * c;
    y = y + x;
    x = x * r;
    return y;
}

// ---- tap sizes ------------------------------------------------------------------------------------
// H:1169  delay + (lfoVal * depth * delay) + 1            (unsigned delay -> double)
MXG_HD int fx_flanger_size(uint32_t delay, double lfo, double depth) {
    const double d = (double)delay;
    return fx_cvt_i32((d + ((lfo * depth) * d)) + 1.0);
}
// H:1207-1208  size1 as the flanger's; size2 = (delay + (lfoVal * depth * delay * 1.02) + 1) * 0.98
MXG_HD int fx_chorus_size2(uint32_t delay, double lfo, double depth) {
    const double d = (double)delay;
    return fx_cvt_i32(((d + (((lfo * depth) * d) * 1.02)) + 1.0) * 0.98);
}

// The size as a bank's ring sees it: <= 0 (and INT_MIN) -> 0, so that the phase resets on every sample as the
// reference's `phase >= size` does; above the bank's `cap` slots -> cap, counted in *ovf (the one defined
// departure: the reference indexes past its own 705 600-slot array there).
MXG_HD int fx_ring_size(int s, int cap, uint32_t &ovf) {
    if (s > cap) {
        ovf += 1;
        return cap;
    }
    return s < 0 ? 0 : s;
}

// One step of dl's phase (C:421-426): the slot it reads and writes.  The test is unsigned so that an uploaded
// negative phase restarts at slot 0 rather than indexing before the ring.  ph < sz <= cap <= 2^31-1: no overflow.
MXG_HD int fx_ring_slot(int &ph, int sz) {
    if ((unsigned)ph >= (unsigned)sz) ph = 0;
    return ph++;
}

MXG_HD double fx_ring_update(double cur, double in, double fb) { return (cur * fb) + (in * fb) * 0.5; }  // C:425

MXG_HD double fx_flanger_out(double o, double in) {  // H:1170-1171
    const double normalise = (1 - fabs(o));
    o *= normalise;
    return (o + in) / 2.0;
}

MXG_HD double fx_chorus_out(double o1, double o2, double in) {  // H:1209-1211
    o1 *= (1.0 - fabs(o1));
    o2 *= (1.0 - fabs(o2));
    return (o1 + o2 + in) / 3.0;
}

// ---- the time-tile classifier ---------------------------------------------------------------------
// Within a tile of T consecutive samples a voice's slots are p0, p0+1, ... until the first reset, then runs
// that all start at 0.  So the touched set is at most two runs, [a0, a0+k) and [0, m) with m <= T (m = the
// longest run after a reset).  The tile is conflict-free -- every slot touched once, all T read-modify-writes
// independent -- iff it has no reset, or one reset and the runs are disjoint (a0 >= m).
struct FxTile {
    int a0, k, m, resets;
    int cur;  // length of the run in progress after the last reset
};

MXG_HD void fx_tile_begin(FxTile &t) { t.a0 = 0; t.k = 0; t.m = 0; t.resets = 0; t.cur = 0; }

// feed the slot of sample i (i = 0, 1, ...) of the tile
MXG_HD void fx_tile_add(FxTile &t, int i, int slot) {
    if (i == 0) {
        t.a0 = slot;
        t.k = 1;
    } else if (t.resets == 0 && slot == t.a0 + t.k) {
        t.k += 1;
    } else if (slot == 0) {  // a reset (no slot after one is ever 0 otherwise: runs go up by one)
        t.resets += 1;
        t.cur = 1;
        if (t.m < 1) t.m = 1;
    } else {
        t.cur += 1;
        if (t.m < t.cur) t.m = t.cur;
    }
}

MXG_HD bool fx_tile_conflict(const FxTile &t) { return t.resets >= 2 || (t.resets == 1 && t.a0 < t.m); }

// Where slot s lives in a tile's 2T-entry staging buffer: [0, m) at T + s, the rest of [a0, a0+k) at s - a0.
// Injective on the touched set; a slot of both runs (a conflicted tile) has one home.
MXG_HD int fx_stage_index(const FxTile &t, int s, int T) { return s < t.m ? T + s : s - t.a0; }

// Which slot lane j stages from each run (-1: none).  Together they cover the touched set exactly once.
MXG_HD int fx_stage_slot_a(const FxTile &t, int j) { return (j < t.k && t.a0 + j >= t.m) ? t.a0 + j : -1; }
MXG_HD int fx_stage_slot_b(const FxTile &t, int j) { return j < t.m ? j : -1; }

}  // namespace
}  // namespace mxg
