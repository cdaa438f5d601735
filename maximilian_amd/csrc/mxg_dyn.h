// mxg_dyn.h -- maxiRingBuf (H:424-494), maxiRMS (H:2579-2616) and maxiDynamics::play (H:2668-2761) as plain per-sample
// arithmetic over a small state struct.  No device state: the same text compiles for the host (tests/host_dyn.cpp,
// which is the checker of the GPU tests), where log10 / pow / sqrt are the host libm's, as in the reference.
//
// What is reproduced is what the reference computes (H = src/maximilian.h):
//   * the detector level is fabs(control) (PEAK; the reference's unqualified abs is the double overload) or the
//     running-sum RMS, in the reference's order: push s*s, running += s*s, running -= tail(window), sqrt(running / window);
//   * controlDB = log10(level) * 20, outDB STARTS as log10(sig) * 20 -- NaN for sig < 0, -inf for 0 -- and is only
//     replaced where a section's comparison holds.  pow(10, NaN * 0.05) > 0 is false: the output is then exactly 0.0
//     and the look-ahead ring is NOT pushed, so its write position depends on the data;
//   * knee forms compare with >= / <, no-knee forms with > / <; each enabled section ticks its envelope once per
//     sample with trigger +1 or -1; the low section uses the plain ratioLow (its envelope runs, its value is unused);
//   * the final scale is control / outAmp.
// Rings are addressed as buf[slot * stride + voice] (slot-major [cap][V] on the device, stride = V).
#pragma once
#include <math.h>
#include <stdint.h>

#include "mxg_envgen.h"
#include "mxg_hd.h"

#define MXG_DYN_PEAK 0
#define MXG_DYN_RMS 1

namespace mxg {
namespace {

// ---- maxiRingBuf ---------------------------------------------------------------------------------
MXG_HD int dyn_ring_advance(int idx, int size) {  // push(): H:434-440, the slot written is the old idx
    idx++;
    return idx == size ? 0 : idx;
}
MXG_HD int dyn_ring_tail_slot(int idx, int size, int n) {  // tail(N): H:449-458 (n <= size)
    return idx >= n ? idx - n : size - (n - idx);
}
MXG_HD int dyn_ring_head_slot(int idx, int size) { return idx == 0 ? size - 1 : idx - 1; }  // head(): H:446

// ---- maxiRMS::play (H:2604-2610) -----------------------------------------------------------------
MXG_HD double dyn_rms_step(double *ring, size_t stride, int size, int &idx, double &running, int window, double s) {
    const double p2 = s * s;
    ring[(size_t)idx * stride] = p2;
    idx = dyn_ring_advance(idx, size);
    running += p2;
    running -= ring[(size_t)dyn_ring_tail_slot(idx, size, window) * stride];
    return sqrt(running / (double)(size_t)window);
}

MXG_HD double dyn_amp_to_db(double a) { return log10(a) * 20.0; }   // maxiConvert::ampToDbs H:955
MXG_HD double dyn_db_to_amp(double d) { return pow(10.0, d * 0.05); }  // maxiConvert::dbsToAmp H:959

MXG_HD double dyn_env_to_ratio(double env, double ratio) {  // H:2887-2895
    return ratio > 1 ? 1 + ((ratio - 1) * env) : 1 - ((1 - ratio) * env);
}

struct DynState {
    EgState eh, el;  // arEnvHigh, arEnvLow
    double running;  // maxiRMS::runningRMS
    int rpos, lpos;  // maxiRingBuf::idx of the RMS ring / of the look-ahead ring
};

struct DynCfg {
    const double *tab_h, *tab_l;  // [3][6] stage tables of the two setupASR envelopes
    long long S;                  // their stage count
    double *rring, *lring;        // this voice's column of the two rings
    size_t stride;
    int cap_r, cap_l;
    int window, look, analyser;   // already clamped to the capacities
};

MXG_HD double dyn_detect(DynState &s, const DynCfg &c, double control) {
    if (c.analyser == MXG_DYN_PEAK) return fabs(control);
    return dyn_rms_step(c.rring, c.stride, c.cap_r, s.rpos, s.running, c.window, control);
}

// The gain computer: detector level in dB -> outDB, ticking the envelopes (H:2674-2747).  out_db enters as ampToDbs(sig).
MXG_HD double dyn_gain(DynState &s, const DynCfg &c, double cdb, double out_db, double th, double rh, double kh, double tl,
                       double rl, double kl) {
    if (rh > 0) {
        if (kh > 0) {
            const double lo = th - (kh / 2.0), hi = th + (kh / 2.0);
            double er = 1;
            if (cdb >= lo) er = dyn_env_to_ratio(envgen_tick(s.eh, c.tab_h, c.S, false, false, 1.0), rh);
            else envgen_tick(s.eh, c.tab_h, c.S, false, false, -1.0);
            if ((cdb >= lo) && (cdb < hi)) {
                const double knee_out = ((hi - th) / er) + th;
                const double range = knee_out - lo;
                const double t = (cdb - lo) / kh;
                const double curve = rh > 1 ? 0.8 : 0.2;
                const double kx = (2 * (1 - t) * t * curve) + (t * t);
                out_db = lo + (kx * range);
            } else if (cdb >= hi) {
                out_db = ((cdb - th) / er) + th;
            }
        } else if (cdb > th) {
            const double er = dyn_env_to_ratio(envgen_tick(s.eh, c.tab_h, c.S, false, false, 1.0), rh);
            out_db = ((cdb - th) / er) + th;
        } else {
            envgen_tick(s.eh, c.tab_h, c.S, false, false, -1.0);
        }
    }
    if (rl > 0) {
        if (kl > 0) {
            const double lo = tl - (kl / 2.0), hi = tl + (kl / 2.0);
            envgen_tick(s.el, c.tab_l, c.S, false, false, cdb < lo ? 1.0 : -1.0);
            if ((cdb >= lo) && (cdb < hi)) {
                const double knee_out = tl - ((tl - lo) / rl);
                const double range = hi - knee_out;
                const double t = (cdb - lo) / kl;
                const double curve = rl > 1 ? 0.2 : 0.8;
                const double kx = (2 * (1 - t) * t * curve) + (t * t);
                out_db = knee_out + (kx * range);
            } else if (cdb < lo) {
                out_db = tl - ((tl - cdb) / rl);
            }
        } else if (cdb < tl) {
            envgen_tick(s.el, c.tab_l, c.S, false, false, 1.0);
            out_db = tl - ((tl - cdb) / rl);
        } else {
            envgen_tick(s.el, c.tab_l, c.S, false, false, -1.0);
        }
    }
    return out_db;
}

// The output stage (H:2749-2760): the conditional look-ahead push and the final scale.
MXG_HD double dyn_output(DynState &s, const DynCfg &c, double sig, double control, double out_amp) {
    double o = 0;
    if (out_amp > 0) {
        if (c.look > 0) {
            c.lring[(size_t)s.lpos * c.stride] = sig;
            s.lpos = dyn_ring_advance(s.lpos, c.cap_l);
            o = c.lring[(size_t)dyn_ring_tail_slot(s.lpos, c.cap_l, c.look) * c.stride];
        } else {
            o = sig;
        }
        o = o * (control / out_amp);
    }
    return o;
}

// maxiDynamics::play, whole.  level_db (may be null) receives the detector level in dB.
MXG_HD double dyn_play(DynState &s, const DynCfg &c, double sig, double control, double th, double rh, double kh, double tl,
                       double rl, double kl, double *level_db) {
    const double cdb = dyn_amp_to_db(dyn_detect(s, c, control));
    if (level_db) *level_db = cdb;
    const double out_db = dyn_gain(s, c, cdb, dyn_amp_to_db(sig), th, rh, kh, tl, rl, kl);
    return dyn_output(s, c, sig, control, dyn_db_to_amp(out_db));
}

// ---- one voice, one block: what a lane of dyn.hip's kernel and a loop iteration of tests/host_dyn.cpp both run ----
#define MXG_DYN_PS_THRESHOLD_HIGH 1
#define MXG_DYN_PS_RATIO_HIGH 2
#define MXG_DYN_PS_KNEE_HIGH 4
#define MXG_DYN_PS_THRESHOLD_LOW 8
#define MXG_DYN_PS_RATIO_LOW 16
#define MXG_DYN_PS_KNEE_LOW 32
#define MXG_DYN_PS_ALL 63

struct DynArgs {
    size_t V, N;
    const double *sig, *control;     // [N][V]; the same pointer = read once
    const double *par[6];            // thresholdHigh, ratioHigh, kneeHigh, thresholdLow, ratioLow, kneeLow
    int ps;                          // MXG_DYN_PS_* bits: that parameter is [N][V], else [V]
    const uint32_t *window, *look;   // [V], in samples
    const int32_t *analyser;         // [V], MXG_DYN_PEAK / MXG_DYN_RMS
    const double *tab_h, *tab_l;     // [nstages][6]
    int nstages;
    double *rring;                   // [cap_r][V]
    int cap_r;
    double *lring;                   // [cap_l][V]
    int cap_l;
    int32_t *rpos, *lpos;            // [V]
    double *running;                 // [V]
    double *dst_h;                   // [5][V]
    int64_t *ist_h;                  // [7][V]
    double *dst_l;
    int64_t *ist_l;
    uint32_t *ovf;                   // [V] or null
    double *out, *level_db;          // [N][V]; level_db may be null
};

// a ring position as stored: anything outside the ring (an uploaded state) restarts at slot 0
MXG_HD int dyn_ring_pos(int32_t p, int cap) { return (p >= 0 && p < cap) ? p : 0; }

MXG_HD void dyn_voice_block(const DynArgs &A, size_t v, const double *tab_h, const double *tab_l) {
    const size_t V = A.V;
    DynState s;
    envgen_load(s.eh, V, v, A.dst_h, A.ist_h);
    envgen_load(s.el, V, v, A.dst_l, A.ist_l);
    s.running = A.running[v];
    s.rpos = dyn_ring_pos(A.rpos[v], A.cap_r);
    s.lpos = dyn_ring_pos(A.lpos[v], A.cap_l);
    uint32_t w = A.window[v], la = A.look[v], over = 0;
    if (w > (uint32_t)A.cap_r) { w = (uint32_t)A.cap_r; over++; }
    if (la > (uint32_t)A.cap_l) { la = (uint32_t)A.cap_l; over++; }
    const DynCfg c = {tab_h, tab_l, A.nstages, A.rring + v, A.lring + v, V, A.cap_r, A.cap_l, (int)w, (int)la,
                      A.analyser[v] == MXG_DYN_PEAK ? MXG_DYN_PEAK : MXG_DYN_RMS};
    double p[6];
#pragma unroll
    for (int k = 0; k < 6; k++) p[k] = (A.ps >> k & 1) ? 0.0 : A.par[k][v];
    const bool same = A.sig == A.control;
    for (size_t n = 0; n < A.N; n++) {
        const size_t e = n * V + v;
#pragma unroll
        for (int k = 0; k < 6; k++)
            if (A.ps >> k & 1) p[k] = A.par[k][e];
        const double sig = A.sig[e];
        const double control = same ? sig : A.control[e];
        double db;
        A.out[e] = dyn_play(s, c, sig, control, p[0], p[1], p[2], p[3], p[4], p[5], &db);
        if (A.level_db) A.level_db[e] = db;
    }
    envgen_store(s.eh, A.nstages, V, v, A.dst_h, A.ist_h);
    envgen_store(s.el, A.nstages, V, v, A.dst_l, A.ist_l);
    A.running[v] = s.running;
    A.rpos[v] = s.rpos;
    A.lpos[v] = s.lpos;
    if (A.ovf) A.ovf[v] += over;
}

struct RmsArgs {
    size_t V, N;
    const double *in;        // [N][V]
    const uint32_t *window;  // [V]
    double *ring;            // [cap][V]
    int cap;
    int32_t *pos;            // [V]
    double *running;         // [V]
    uint32_t *ovf;
    double *out;
};

MXG_HD void rms_voice_block(const RmsArgs &A, size_t v) {
    const size_t V = A.V;
    int pos = dyn_ring_pos(A.pos[v], A.cap);
    double running = A.running[v];
    uint32_t w = A.window[v], over = 0;
    if (w > (uint32_t)A.cap) { w = (uint32_t)A.cap; over++; }
    for (size_t n = 0; n < A.N; n++)
        A.out[n * V + v] = dyn_rms_step(A.ring + v, V, A.cap, pos, running, (int)w, A.in[n * V + v]);
    A.pos[v] = pos;
    A.running[v] = running;
    if (A.ovf) A.ovf[v] += over;
}

// maxiEnvGen::setTime(index, ms) (H:2449-2462 with setupSegmentTime H:2532-2546, accumulatedTime = 0) on one row of the
// [S][6] table (startlevel, endlevel, gradient, curve, length, hold).  Returns the reference's `error`.
MXG_HD int dyn_envgen_set_time(double *tab, size_t S, size_t index, double ms, double sr) {
    const double HOLD = -46692.0;
    if (index >= S) return 1;  // (index == S passes the reference's test and writes past its vector: refused here)
    bool contains_hold = false;
    for (size_t i = 0; i < S; i++) contains_hold = contains_hold || tab[6 * i + 5] != 0;
    if (ms == HOLD && contains_hold) return 1;
    double *st = tab + 6 * index;
    if (ms == HOLD) {
        st[4] = 0; st[5] = 1; st[2] = 0;
    } else {
        const double len = ((ms / 1000.0) * sr) + 0.0;
        const size_t l = (size_t)floor(len);
        st[4] = (double)l; st[2] = 1.0 / l; st[5] = 0;
    }
    return 0;
}

}  // namespace
}  // namespace mxg
