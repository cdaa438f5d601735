// mxg_classic.h -- the last per-sample classes of the reference's core header as plain arithmetic: maxiDyn::gate / compressor /
// compress (C:1200-1298), maxiEnvelope::line / trigger (C:377-412), maxiLagExp<double>::addSample (H:523-526), maxiMap::linlin /
// linexp / explin / clamp (H:801-854) and maxiConvert::ampToDbs / dbsToAmp (H:955-961).  C = src/maximilian.cpp, H =
// src/maximilian.h.  No device state: the same text compiles for the host (tests/host_classic.cpp, the mxg_*_host entry points)
// and for the kernels of classic.hip (K23).  One step function per reference call, the reference's expression trees, never contracted into
// an FMA.
//
// What is reproduced is what the reference computes:
//   * the gate: the five ifs in the reference's order; `output` persists when no branch writes it; amplitude == 0 -> 0.01 on the
//     first attack; holdcount == holdtime fires on every sample it holds (a fresh object with holdtime 0 included);
//     output = input * (amplitude *= release);
//   * the compressor: currentRatio == 0 -> ratio; the attack runs while currentRatio < ratio - 1 and the release phase is
//     entered in the same call; input / (1. + currentRatio); the make-up factor 1 + log(ratio) is an INPUT (cls_makeup with the
//     host libm), so the step has no transcendental;
//   * the envelope: period = 4. / (segments[valindex + 1] * 0.0044), the two increments, the valindex > n - 1 reset to n - 2 and
//     the advance; output = 0 while not playing.  period, sampleRate / period and the two increments depend on the table, the
//     sample rate, valindex and startval only; they are formed where one of those changes (env_load / env_incs) by the
//     reference's own expressions, so the values added per sample are the reference's bits.  The reference also reads
//     segments[valindex + 2] into a member nothing uses, and for one call after the last segment segments[n] and segments[n + 1]
//     into values no taken branch uses: those reads are not made.  Every table index is held inside [0, n - 1] (one defined
//     departure, below);
//   * the lag: val = (alpha * x) + (alphaReciprocal * val), alpha and alphaReciprocal independent;
//   * the maps: the clip max(min(val, inMax), inMin) as std::min / std::max compare (a NaN val stays, -0.0 and a reversed range
//     behave as the compares leave them), clamp as if / else if.
// Departures: a table index that the reference would take outside its vector (an odd start index walks to n - 1 and reads
// segments[n] as a time; a trigger index outside [0, n - 2]) is held inside the table.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

#define MXG_MAP_LINLIN 0
#define MXG_MAP_LINEXP 1
#define MXG_MAP_EXPLIN 2
#define MXG_MAP_CLAMP 3
#define MXG_MAP_AMPTODBS 4
#define MXG_MAP_DBSTOAMP 5
#define MXG_MAP_MODES 6
#define MXG_ENVELOPE_MAX_S 64

namespace mxg {
namespace {

// ---- maxiDyn ---------------------------------------------------------------------------------------------------------
// the members gate() and compressor() share; fresh: all zero (static-storage semantics)
struct ClsDyn {
    double amplitude, currentRatio, output;
    int64_t holdcount;
    int attackphase, holdphase, releasephase;
};

MXG_HD double cls_gate(ClsDyn &s, double input, double threshold, int64_t holdtime, double attack, double release) {
    if (fabs(input) > threshold && s.attackphase != 1) {
        s.holdcount = 0;
        s.releasephase = 0;
        s.attackphase = 1;
        if (s.amplitude == 0) s.amplitude = 0.01;
    }
    if (s.attackphase == 1 && s.amplitude < 1) {
        s.amplitude *= (1 + attack);
        s.output = input * s.amplitude;
    }
    if (s.amplitude >= 1) {
        s.attackphase = 0;
        s.holdphase = 1;
    }
    if (s.holdcount < holdtime && s.holdphase == 1) {
        s.output = input;
        s.holdcount++;
    }
    if (s.holdcount == holdtime) {
        s.holdphase = 0;
        s.releasephase = 1;
    }
    if (s.releasephase == 1 && s.amplitude > 0.) {
        s.amplitude *= release;
        s.output = input * s.amplitude;
    }
    return s.output;
}

// 1 + log(ratio) with the caller's libm (host: the reference's own expression)
MXG_HD double cls_makeup(double ratio) { return 1 + log(ratio); }
// maxiDyn::setAttack / setRelease: pow(0.01, 1.0 / (ms * sampleRate * 0.001)) -- which compress() then uses as 1 + attack
MXG_HD double cls_dyn_coeff(double ms, double sampleRate) { return pow(0.01, 1.0 / (ms * sampleRate * 0.001)); }

MXG_HD double cls_compress(ClsDyn &s, double input, double ratio, double makeup, double threshold, double attack, double release) {
    if (fabs(input) > threshold && s.attackphase != 1) {
        s.holdcount = 0;
        s.releasephase = 0;
        s.attackphase = 1;
        if (s.currentRatio == 0) s.currentRatio = ratio;
    }
    if (s.attackphase == 1 && s.currentRatio < ratio - 1) {
        s.currentRatio *= (1 + attack);
    }
    if (s.currentRatio >= ratio - 1) {
        s.attackphase = 0;
        s.releasephase = 1;
    }
    if (s.releasephase == 1 && s.currentRatio > 0.) {
        s.currentRatio *= release;
    }
    s.output = input / (1. + s.currentRatio);  // (both branches of the reference's input > 0. are this expression)
    return s.output * makeup;
}

// ---- maxiEnvelope ----------------------------------------------------------------------------------------------------
struct ClsEnv {
    double amplitude, startval;
    int valindex, isPlaying;
    // what line() forms from the table at valindex: currentval, sampleRate / period, and the two increments
    double currentval, spp, up, down;
    // what those were formed from: the table index (MXG_ENV_NONE: nothing yet; no int) and the startval of the increments
    int64_t loaded;
    double incstart;
};
#define MXG_ENV_NONE INT64_MIN

// an index into a table of n entries (n >= 1), held inside it
MXG_HD int env_at(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// count[v] is held inside [1, S] (a legal one is 2 .. S)
MXG_HD int cls_env_count(int32_t count, size_t S) { return count < 1 ? 1 : (count > (int32_t)S ? (int32_t)S : count); }

// the increments of the two moving branches: they change with currentval, spp and startval
MXG_HD void env_incs(ClsEnv &s) {
    s.up = ((s.currentval - s.startval) / s.spp);
    s.down = (((s.currentval - s.startval) * (-1)) / s.spp);
    s.incstart = s.startval;
}

// Before a line() call: segments[valindex] and segments[valindex + 1] of a table with `stride` doubles between its entries, and
// what line() forms from them.  With valindex >= n nothing of it reaches a result (both moving branches ask for valindex < n,
// the advance is not reached), so nothing is read; an index that was loaded last time is not loaded again (the end-of-table
// oscillation n -> n - 2 -> n comes back to the same entries on every second call), and the increments are formed again only
// where startval moved.  Same inputs, same expressions: the reference's bits.
MXG_HD void env_load(ClsEnv &s, const double *seg, size_t stride, int n, double sampleRate) {
    if (s.valindex >= n) return;
    if (s.valindex != s.loaded) {
        const int i = env_at(s.valindex, n), j = i + 1 > n - 1 ? n - 1 : i + 1;
        const double period = 4. / (seg[(size_t)j * stride] * 0.0044);
        s.currentval = seg[(size_t)i * stride];
        s.spp = sampleRate / period;
        s.loaded = s.valindex;
        env_incs(s);
    } else if (!(s.startval == s.incstart)) {
        env_incs(s);
    }
}

MXG_HD void cls_env_trigger(ClsEnv &s, int index, double amp, int n) {
    s.isPlaying = 1;
    s.valindex = index < 0 ? 0 : (index > n - 2 ? (n - 2 < 0 ? 0 : n - 2) : index);  // held inside [0, n - 2]
    s.amplitude = amp;
}

// one line() call; true: valindex changed, the caller runs env_load before the next call
MXG_HD bool cls_env_line(ClsEnv &s, int n, double &out) {
    bool moved = false;
    if (s.isPlaying == 1) {
        if (s.currentval - s.amplitude > 0.0000001 && s.valindex < n) {
            s.amplitude += s.up;
        } else if (s.currentval - s.amplitude < -0.0000001 && s.valindex < n) {
            s.amplitude -= s.down;
        } else if (s.valindex > n - 1) {
            s.valindex = n - 2;
            moved = true;
        } else {
            s.valindex = s.valindex + 2;
            s.startval = s.currentval;
            moved = true;
        }
        out = s.amplitude;
    } else {
        out = 0;
    }
    return moved;
}

// ---- maxiLagExp<double> ----------------------------------------------------------------------------------------------
MXG_HD double cls_lag(double val, double alpha, double alphaReciprocal, double x) { return (alpha * x) + (alphaReciprocal * val); }

// ---- maxiMap / maxiConvert -------------------------------------------------------------------------------------------
// std::max(std::min(val, inMax), inMin): min(a, b) = b < a ? b : a, max(a, b) = a < b ? b : a
MXG_HD double cls_clip(double val, double inMin, double inMax) {
    const double m = inMax < val ? inMax : val;
    return m < inMin ? inMin : m;
}
MXG_HD double cls_linlin(double val, double inMin, double inMax, double outMin, double outMax) {
    val = cls_clip(val, inMin, inMax);
    return ((val - inMin) / (inMax - inMin) * (outMax - outMin)) + outMin;
}
MXG_HD double cls_linexp(double val, double inMin, double inMax, double outMin, double outMax) {
    val = cls_clip(val, inMin, inMax);
    return pow((outMax / outMin), (val - inMin) / (inMax - inMin)) * outMin;
}
// log(inMax / inMin) of explin with the caller's libm
MXG_HD double cls_explin_den(double inMin, double inMax) { return log(inMax / inMin); }
MXG_HD double cls_explin(double val, double inMin, double inMax, double outMin, double outMax, double den) {
    val = cls_clip(val, inMin, inMax);
    return (log(val / inMin) / den * (outMax - outMin)) + outMin;
}
MXG_HD double cls_clamp(double v, double low, double high) {
    if (v > high) v = high;
    else if (v < low) v = low;
    return v;
}
MXG_HD double cls_amptodbs(double amp) { return log10(amp) * 20.0; }
MXG_HD double cls_dbstoamp(double dbs) { return pow(10.0, dbs * 0.05); }

// one element of `mode`; r0 .. r3 = inMin, inMax, outMin, outMax (clamp: low, high), aux = cls_explin_den (explin only)
template <int MODE>
MXG_HD double cls_map(double x, double r0, double r1, double r2, double r3, double aux) {
    if (MODE == MXG_MAP_LINLIN) return cls_linlin(x, r0, r1, r2, r3);
    if (MODE == MXG_MAP_LINEXP) return cls_linexp(x, r0, r1, r2, r3);
    if (MODE == MXG_MAP_EXPLIN) return cls_explin(x, r0, r1, r2, r3, aux);
    if (MODE == MXG_MAP_CLAMP) return cls_clamp(x, r0, r1);
    if (MODE == MXG_MAP_AMPTODBS) return cls_amptodbs(x);
    return cls_dbstoamp(x);
}

// ---- whole blocks on host arrays, in the layouts of the mxg_*_render entry points (include/maxigpu.h) --------------------
// (the bodies of the mxg_*_host entry points and of tests/host_classic.cpp; ps_flags / strides as the kernels read them)
#define MXG_CLASSIC_PS_THRESHOLD 1
#define MXG_CLASSIC_PS_ATTACK 2
#define MXG_CLASSIC_PS_RELEASE 4
#define MXG_CLASSIC_PS_RATIO 8
#define MXG_CLASSIC_PS_MASK 15

static inline ClsDyn cls_dyn_get(size_t V, size_t v, const double *dst, const int64_t *ist) {
    return {dst[v], dst[V + v], dst[2 * V + v], ist[v], (int)ist[V + v], (int)ist[2 * V + v], (int)ist[3 * V + v]};
}
static inline void cls_dyn_put(const ClsDyn &s, size_t V, size_t v, double *dst, int64_t *ist) {
    dst[v] = s.amplitude; dst[V + v] = s.currentRatio; dst[2 * V + v] = s.output;
    ist[v] = s.holdcount; ist[V + v] = s.attackphase; ist[2 * V + v] = s.holdphase; ist[3 * V + v] = s.releasephase;
}

static inline void cls_host_gate(size_t V, size_t N, const double *in, const double *thr, const double *att, const double *rel, int ps,
                                 const int64_t *holdtime, double *dst, int64_t *ist, double *out) {
    const size_t st = (ps & MXG_CLASSIC_PS_THRESHOLD) ? V : 0, sa = (ps & MXG_CLASSIC_PS_ATTACK) ? V : 0, sr = (ps & MXG_CLASSIC_PS_RELEASE) ? V : 0;
    for (size_t v = 0; v < V; v++) {
        ClsDyn s = cls_dyn_get(V, v, dst, ist);
        for (size_t n = 0; n < N; n++) out[n * V + v] = cls_gate(s, in[n * V + v], thr[n * st + v], holdtime[v], att[n * sa + v], rel[n * sr + v]);
        cls_dyn_put(s, V, v, dst, ist);
    }
}

static inline void cls_host_compress(size_t V, size_t N, const double *in, const double *ratio, const double *makeup, const double *thr,
                                     const double *att, const double *rel, int ps, double *dst, int64_t *ist, double *out) {
    const size_t st = (ps & MXG_CLASSIC_PS_THRESHOLD) ? V : 0, sa = (ps & MXG_CLASSIC_PS_ATTACK) ? V : 0, sr = (ps & MXG_CLASSIC_PS_RELEASE) ? V : 0;
    const size_t sq = (ps & MXG_CLASSIC_PS_RATIO) ? V : 0;
    for (size_t v = 0; v < V; v++) {
        ClsDyn s = cls_dyn_get(V, v, dst, ist);
        for (size_t n = 0; n < N; n++)
            out[n * V + v] = cls_compress(s, in[n * V + v], ratio[n * sq + v], makeup[n * sq + v], thr[n * st + v], att[n * sa + v], rel[n * sr + v]);
        cls_dyn_put(s, V, v, dst, ist);
    }
}

static inline void cls_host_line(size_t V, size_t N, size_t S, const double *seg, const int32_t *count, const double *trig,
                                 const int32_t *trig_index, const double *trig_amp, double sampleRate, double *dst, int32_t *ist, double *out) {
    for (size_t v = 0; v < V; v++) {
        const int n = cls_env_count(count[v], S);
        ClsEnv s = {dst[v], dst[V + v], ist[v], ist[V + v], 0, 0, 0, 0, MXG_ENV_NONE, 0};
        env_load(s, seg + v, V, n, sampleRate);
        for (size_t i = 0; i < N; i++) {
            if (trig && trig[i * V + v] != 0.0) {
                cls_env_trigger(s, trig_index[v], trig_amp[v], n);
                env_load(s, seg + v, V, n, sampleRate);
            }
            if (cls_env_line(s, n, out[i * V + v])) env_load(s, seg + v, V, n, sampleRate);
        }
        dst[v] = s.amplitude; dst[V + v] = s.startval; ist[v] = s.valindex; ist[V + v] = s.isPlaying;
    }
}

static inline void cls_host_lag(size_t V, size_t N, const double *in, const double *alpha, const double *recip, int ps, double *val, double *out) {
    const size_t sa = ps ? V : 0;
    for (size_t v = 0; v < V; v++) {
        double y = val[v];
        for (size_t n = 0; n < N; n++) out[n * V + v] = y = cls_lag(y, alpha[n * sa + v], recip[n * sa + v], in[n * V + v]);
        val[v] = y;
    }
}

static inline int cls_host_map(int mode, size_t V, size_t N, const double *in, const double *range, const double *aux, double *out) {
    for (size_t e = 0; e < N * V; e++) {
        const size_t v = e % V;
        const bool ranged = mode <= MXG_MAP_CLAMP;
        const double r0 = ranged ? range[v] : 0.0, r1 = ranged ? range[V + v] : 0.0;
        const double r2 = mode <= MXG_MAP_EXPLIN ? range[2 * V + v] : 0.0, r3 = mode <= MXG_MAP_EXPLIN ? range[3 * V + v] : 0.0;
        const double a = mode == MXG_MAP_EXPLIN ? aux[v] : 0.0;
        switch (mode) {
            case MXG_MAP_LINLIN: out[e] = cls_map<MXG_MAP_LINLIN>(in[e], r0, r1, r2, r3, a); break;
            case MXG_MAP_LINEXP: out[e] = cls_map<MXG_MAP_LINEXP>(in[e], r0, r1, r2, r3, a); break;
            case MXG_MAP_EXPLIN: out[e] = cls_map<MXG_MAP_EXPLIN>(in[e], r0, r1, r2, r3, a); break;
            case MXG_MAP_CLAMP: out[e] = cls_map<MXG_MAP_CLAMP>(in[e], r0, r1, r2, r3, a); break;
            case MXG_MAP_AMPTODBS: out[e] = cls_map<MXG_MAP_AMPTODBS>(in[e], r0, r1, r2, r3, a); break;
            case MXG_MAP_DBSTOAMP: out[e] = cls_map<MXG_MAP_DBSTOAMP>(in[e], r0, r1, r2, r3, a); break;
            default: return -1;
        }
    }
    return 0;
}

}  // namespace
}  // namespace mxg
