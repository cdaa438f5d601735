// mxg_reverb.h -- maxiSatReverb, maxiFreeVerb and maxiFreeVerbStereo (reference src/libs/maxiReverb.h / .cpp, the one-pole
// low-pass of maxiFilter::lopass in src/maximilian.cpp) as plain per-sample arithmetic, the topology tables, the slot
// arithmetic reverb.hip's time tiles are built on, and a step-by-step walk of one voice (rv_voice_ref) over the same
// state layout as the kernel.  Only + - * and compares: the same text compiles for the host (tests/host_reverb.cpp),
// where rv_voice_ref is the checker of the GPU tests.  Compile with contraction off.
//
// What the reference computes.  Every filter owns a ring and an index that starts at 0 and goes
// idx = (idx != D-1) ? idx+1 : 0 with the same D on every call, so a ring of exactly D slots is equivalent:
//   comb (plain):    d = ring[idx]; o = x + (0.85 * d);                          ring[idx] = o
//   comb (low-pass): d = ring[idx]; y = y + (1.0 - cut) * (d - y); o = x + (w * y); ring[idx] = o
//   allpass:         d = ring[idx]; t = t + d * 0.85; o = d + (t * (-0.85));       ring[idx] = t
//   comb sum:        acc = 0.0; acc += comb_i(x) in order;  allpass chain: t = allpass_j(t) in order
// maxiSatReverb::play      = allpasses(combs_plain(x, 4), 3)            (the constructor's gains are stored, never used)
// maxiFreeVerb::play(x)    = allpasses(combs_lowpass(x, 8), 4)          with the object's w, cut (fresh: 0.84, 0.2)
// maxiFreeVerb::play(x,r,a): w = clamp01(r*0.10 + 0.84), cut = clamp01(a), persistently; then 8 combs and 31 allpasses
// maxiFreeVerbStereo       : left = allpasses(combs_plain(x, 8), 4); right = allpasses(0.0, 4) on the SAME four rings, a
//                            second step in the same sample (its comb sum runs no comb, its chain ignores `firstfilter`);
//                            roomsize and absorbtion are stored and read by nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

namespace mxg {
namespace {

constexpr int RV_SAT = 0, RV_FREEVERB = 1, RV_STEREO = 2;  // = MXG_REVERB_SAT / _FREEVERB / _FREEVERB_STEREO
constexpr int RV_PS_ROOM = 1, RV_PS_ABSORB = 2;            // = MXG_REVERB_PS_ROOMSIZE / _ABSORBTION
constexpr int RV_MAX_FILTERS = 39;
constexpr int RV_LP = 8;  // low-pass states per voice

// ---- topology: delay lengths in samples (independent of the sample rate) --------------------------------------------
MXG_HD constexpr int rv_ncomb(int kind) { return kind == RV_SAT ? 4 : 8; }
MXG_HD constexpr int rv_nap(int kind) { return kind == RV_SAT ? 3 : kind == RV_FREEVERB ? 31 : 4; }
MXG_HD constexpr int rv_nfilt(int kind) { return rv_ncomb(kind) + rv_nap(kind); }
MXG_HD constexpr int rv_steps(int kind) { return kind == RV_STEREO ? 2 : 1; }  // allpass steps per sample
MXG_HD constexpr int rv_comb_len(int kind, int c) {
    return kind == RV_SAT ? (c == 0 ? 778 : c == 1 ? 901 : c == 2 ? 1011 : 1123)
                          : (c == 0 ? 1557 : c == 1 ? 1617 : c == 2 ? 1491 : c == 3 ? 1422 : c == 4 ? 1277 : c == 5 ? 1356
                             : c == 6 ? 1188 : 1116);
}
MXG_HD constexpr int rv_ap_len(int kind, int j) {
    return kind == RV_SAT ? (j == 0 ? 125 : j == 1 ? 42 : 12)
                          : (j == 0 ? 225 : j == 1 ? 556 : j == 2 ? 441 : j == 3 ? 341 : 13 * (j + 1));
}
// filter f of a voice: the combs first, then the allpasses
MXG_HD constexpr int rv_len(int kind, int f) {
    return f < rv_ncomb(kind) ? rv_comb_len(kind, f) : rv_ap_len(kind, f - rv_ncomb(kind));
}
MXG_HD constexpr int rv_off(int kind, int f) {  // first slot of filter f inside the voice's ring area
    int o = 0;
    for (int g = 0; g < f; g++) o += rv_len(kind, g);
    return o;
}
MXG_HD constexpr int rv_ring_doubles(int kind) { return rv_off(kind, rv_nfilt(kind)); }
static_assert(rv_ring_doubles(RV_SAT) == 3992 && rv_ring_doubles(RV_FREEVERB) == 18905 && rv_ring_doubles(RV_STEREO) == 12587,
              "ring state per voice");

// ---- the per-sample arithmetic -----------------------------------------------------------------------------------
MXG_HD double rv_comb_plain(double d, double x) { return x + (0.85 * d); }
MXG_HD double rv_lowpass(double y, double cut, double d) { return y + (1.0 - cut) * (d - y); }
MXG_HD double rv_comb_lp(double x, double w, double y) { return x + (w * y); }
// one allpass step: `t` comes in as the stage's input and leaves as its output; returns what the ring slot gets
MXG_HD double rv_allpass(double d, double &t) {
    const double s = t + d * 0.85;
    t = d + (s * (-0.85));
    return s;
}
MXG_HD double rv_clamp01(double v) {  // a NaN stays a NaN
    if (v > 1.0) v = 1.0;
    if (v < 0.0) v = 0.0;
    return v;
}
MXG_HD double rv_room_w(double roomsize) { return rv_clamp01((roomsize * 0.10) + 0.84); }

// ---- slot arithmetic of a time tile ------------------------------------------------------------------------------
// A stored index outside its ring restarts at slot 0 (the reference cannot produce one).
MXG_HD int rv_idx_fix(int32_t idx, int D) { return (uint32_t)idx < (uint32_t)D ? idx : 0; }
// the slot of the k-th step after `idx`, 0 <= k <= D
MXG_HD int rv_slot(int idx, int k, int D) {
    const int s = idx + k;
    return s >= D ? s - D : s;
}
// the index after k >= 0 steps
MXG_HD int rv_idx_after(int idx, int k, int D) { return (idx + k) % D; }
// Samples a tile may take in one parallel pass over a ring of D slots stepped `steps` times per sample: the steps*L slots
// they touch are distinct iff steps*L <= D.  (D >= steps for every ring here.)
MXG_HD constexpr int rv_sub_len(int D, int steps, int T) { return D / steps < T ? D / steps : T; }

// ---- one voice, one sample at a time, over the bank's state layout ---------------------------------------------------
// rings [V][S] (voice-major, filter f at rv_off(kind, f)), idx int32 [V][F], lp [V][8], wc [V][2] = (w, cut).
// in [N][V]; room / absorb [V], or [N][V] behind their RV_PS_* bit; out [N][V], the stereo kind [2][N][V].
struct RvArgs {
    int mode;  // maxiFreeVerb only: 0 = play(x), 1 = play(x, roomsize, absorbtion)
    size_t V, N;
    const double *in, *room, *absorb;
    int ps;
    double *rings;
    int32_t *idx;
    double *lp, *wc;
    double *out;
};

template <int KIND>
MXG_HD void rv_voice_ref(const RvArgs &A, size_t v) {
    constexpr int NC = rv_ncomb(KIND), F = rv_nfilt(KIND), S = rv_ring_doubles(KIND);
    const size_t V = A.V, N = A.N;
    double *ring = A.rings + v * (size_t)S;
    int off[F], len[F], idx[F];
    for (int f = 0; f < F; f++) {
        off[f] = rv_off(KIND, f);
        len[f] = rv_len(KIND, f);
        idx[f] = rv_idx_fix(A.idx[v * F + f], len[f]);
    }
    double y[RV_LP] = {0, 0, 0, 0, 0, 0, 0, 0}, w = 0.0, cut = 0.0;
    if (KIND == RV_FREEVERB) {
        for (int c = 0; c < RV_LP; c++) y[c] = A.lp[v * RV_LP + c];
        w = A.wc[v * 2];
        cut = A.wc[v * 2 + 1];
    }
    const int nap = KIND == RV_FREEVERB ? (A.mode ? 31 : 4) : rv_nap(KIND);
    for (size_t n = 0; n < N; n++) {
        const double x = A.in[n * V + v];
        if (KIND == RV_FREEVERB && A.mode) {
            w = rv_room_w(A.room[(A.ps & RV_PS_ROOM) ? n * V + v : v]);
            cut = rv_clamp01(A.absorb[(A.ps & RV_PS_ABSORB) ? n * V + v : v]);
        }
        double acc = 0.0;
        for (int c = 0; c < NC; c++) {
            double *slot = ring + off[c] + idx[c];
            double o;
            if (KIND == RV_FREEVERB) {
                y[c] = rv_lowpass(y[c], cut, *slot);
                o = rv_comb_lp(x, w, y[c]);
            } else {
                o = rv_comb_plain(*slot, x);
            }
            *slot = o;
            idx[c] = idx[c] != len[c] - 1 ? idx[c] + 1 : 0;
            acc += o;
        }
        for (int pass = 0; pass < rv_steps(KIND); pass++) {
            double t = pass == 0 ? acc : 0.0;
            for (int f = NC; f < NC + nap; f++) {
                double *slot = ring + off[f] + idx[f];
                *slot = rv_allpass(*slot, t);
                idx[f] = idx[f] != len[f] - 1 ? idx[f] + 1 : 0;
            }
            A.out[(pass * N + n) * V + v] = t;
        }
    }
    for (int f = 0; f < F; f++) A.idx[v * F + f] = idx[f];
    if (KIND == RV_FREEVERB) {
        for (int c = 0; c < RV_LP; c++) A.lp[v * RV_LP + c] = y[c];
        A.wc[v * 2] = w;
        A.wc[v * 2 + 1] = cut;
    }
}

}  // namespace
}  // namespace mxg
