// mxg_shaper.h -- the reference's small stream classes as plain per-sample arithmetic: maxiNonlinearity (H:1046-1137, alias
// maxiDistortion), maxiXFade::xfade (H:1502-1526) over maxiMap::clamp / linlin (H:801-805, 843-854), maxiSelect::play and
// maxiSelectX::play (H:2028-2085) and maxiLine::play / prepare (H:1537-1616).  H = src/maximilian.h.  No device state: the same
// text compiles for the host (tests/host_shaper.cpp) and for the kernels of shaper.hip (K18).  One step function per reference
// call, the reference's expression trees, never contracted into an FMA.
//
// What is reproduced is what the reference computes:
//   * hardclip, fastatan, fastAtanDist: compares, + * / only -- bit-exact.  A NaN falls through every compare and stays a NaN;
//   * softclip: (2 / 3.0) * (x - cube / 3.0) with cube = (x * x) * x where the reference calls pow(x, 3): at most 1 ULP of a value
//     below 1 apart; the clipped branches give exactly +-1;
//   * atanDist: norm * atan(in * shape), norm = 1.0 / atan(shape) (from the host libm for a per-voice shape: mxg_atan_norm_host);
//   * asymclip: the four branches in the reference's order; pow is the platform's (device: tolerance);
//   * xfade: clamp, then linlin's own min / max (std::min / std::max as compares, so a NaN stays a NaN), ((v - -1) / (1 - -1) *
//     (1 - 0)) + 0, the gains sqrt(1.0 - n) and sqrt(n), out = (ch1 * g1) + (ch2 * g2);
//   * select: index *= (K - 1e-9) when normalised; below 0 -> 0, >= K -> K - 1; Select truncates, SelectX takes floor, wraps
//     a2 = a1 + 1 to 0 at K and mixes (v[a1] * (1.0 - mix)) + (v[a2] * mix);
//   * the line: the state machine of play() statement by statement, `triggered` kept as the 0.0 / 1.0 double it is there.
// One defined departure: a NaN index falls through both clamps into a float -> integer cast in the reference (undefined);
// here it is taken as index 0.0 and reported to the caller.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

#define MXG_SHAPE_HARDCLIP 0
#define MXG_SHAPE_SOFTCLIP 1
#define MXG_SHAPE_FASTATAN 2
#define MXG_SHAPE_FASTATANDIST 3
#define MXG_SHAPE_ATANDIST 4
#define MXG_SHAPE_ASYMCLIP 5
#define MXG_SHAPE_MODES 6
#define MXG_SELECT_MAX_K 64
#define MXG_XFADE_MAX_C 8

namespace mxg {
namespace {

// ---- maxiNonlinearity ------------------------------------------------------------------------------------------------
MXG_HD double shp_hardclip(double x) { return x >= 1 ? 1 : (x <= -1 ? -1 : x); }

MXG_HD double shp_softclip(double x) {
    if (x >= 1) return 1;
    if (x <= -1) return -1;
    const double cube = (x * x) * x;  // the reference: pow(x, 3)
    return (2 / 3.0) * (x - cube / 3.0);
}

MXG_HD double shp_fastatan(double x) { return (x / (1.0 + 0.28 * (x * x))); }

MXG_HD double shp_fastatandist(double in, double shape) { return (1.0 / shp_fastatan(shape)) * shp_fastatan(in * shape); }

// 1.0 / atan(shape): the factor of atanDist
MXG_HD double shp_atan_norm(double shape) { return 1.0 / atan(shape); }
MXG_HD double shp_atandist(double in, double shape, double norm) { return norm * atan(in * shape); }

MXG_HD double shp_asymclip(double x, double a, double b) {
    if (x >= 1) x = 1;
    else if (x <= -1) x = -1;
    else if (x < 0) x = -(pow(-x, a));
    else x = pow(x, b);
    return x;
}

// one sample of `mode`; pa = shape / a, pb = the atanDist factor / b (unused ones are ignored)
template <int MODE>
MXG_HD double shp_apply(double x, double pa, double pb) {
    if (MODE == MXG_SHAPE_HARDCLIP) return shp_hardclip(x);
    if (MODE == MXG_SHAPE_SOFTCLIP) return shp_softclip(x);
    if (MODE == MXG_SHAPE_FASTATAN) return shp_fastatan(x);
    if (MODE == MXG_SHAPE_FASTATANDIST) return shp_fastatandist(x, pa);
    if (MODE == MXG_SHAPE_ATANDIST) return shp_atandist(x, pa, pb);
    return shp_asymclip(x, pa, pb);
}

// ---- maxiXFade::xfade ------------------------------------------------------------------------------------------------
MXG_HD void shp_xfade_gains(double xfader, double &g1, double &g2) {
    const double lo = -1, hi = 1, omin = 0, omax = 1;
    xfader = xfader > hi ? hi : (xfader < lo ? lo : xfader);  // maxiMap::clamp
    double val = hi < xfader ? hi : xfader;                    // std::min(val, inMax)
    val = val < lo ? lo : val;                                 // std::max(.., inMin)
    const double n = ((val - lo) / (hi - lo) * (omax - omin)) + omin;
    g1 = sqrt(1.0 - n);
    g2 = sqrt(n);
}
MXG_HD double shp_xfade(double ch1, double ch2, double g1, double g2) { return (ch1 * g1) + (ch2 * g2); }

// ---- maxiSelect / maxiSelectX ----------------------------------------------------------------------------------------
// the scaled and clamped index; *nan: the index was a NaN (taken as 0.0)
MXG_HD double shp_select_index(double index, size_t K, bool normalised, bool *nan) {
    if (normalised) index *= ((double)K - 1e-9);
    if (index < 0) index = 0;
    else if (index >= (double)K) index = (double)(K - 1);
    *nan = index != index;
    return *nan ? 0.0 : index;
}
// maxiSelect: static_cast<size_t>(index)
MXG_HD size_t shp_select_at(double index) { return (size_t)index; }
// maxiSelectX: a1 = floor(index), mix = index - a1, a2 = a1 + 1 wrapping to 0
MXG_HD void shp_selectx_at(double index, size_t K, size_t &a1, size_t &a2, double &mix) {
    a1 = (size_t)floor(index);
    mix = index - (double)a1;
    a2 = a1 + 1;
    if (a2 == K) a2 = 0;
}
MXG_HD double shp_selectx_mix(double v1, double v2, double mix) { return (v1 * (1.0 - mix)) + (v2 * mix); }

// ---- maxiLine --------------------------------------------------------------------------------------------------------
struct LineState {
    double value, last;         // lineValue, lastTrigVal (fresh: 0, -1)
    double triggered;           // 0.0 / 1.0, a double in the reference too
    bool complete;              // lineComplete
};
struct LinePar {
    double start, end, inc;
    bool oneShot, enable;
};

MXG_HD double shp_line(LineState &s, const LinePar &p, double trigger) {
    if (!s.complete) {
        if (p.enable && !(s.triggered != 0.0)) {
            s.triggered = (trigger > 0.0 && s.last <= 0.0) ? 1.0 : 0.0;
            s.value = p.start;
        }
        if (s.triggered != 0.0) {
            s.value += p.inc;
            if (p.inc <= 0) s.complete = s.value <= p.end;
            else s.complete = s.value >= p.end;
            if (s.complete) {
                if (!p.oneShot) {  // reset()
                    s.triggered = 0.0;
                    s.complete = false;
                }
            }
        }
        s.last = trigger;
    }
    return s.value;
}

// maxiLine::prepare: lineValue takes the PREVIOUS lineStart (the reference assigns it before lineStart changes)
MXG_HD void shp_line_prepare(LineState &s, LinePar &p, double start, double end, double durationMs, bool isOneShot, double sampleRate) {
    s.value = p.start;
    p.start = start;
    p.end = end;
    const double lineMag = end - start;
    const double durInSamples = durationMs / 1000.0 * sampleRate;
    p.inc = lineMag / durInSamples;
    p.oneShot = isOneShot;
    s.triggered = 0.0;
    s.complete = false;
}

}  // namespace
}  // namespace mxg
