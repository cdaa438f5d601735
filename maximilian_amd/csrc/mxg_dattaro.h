// mxg_dattaro.h -- maxiDattaroReverb (reference src/libs/maxiReverb.h / .cpp: the constructor and playStereo, the ring
// primitives maxiReverbFilters::onetap / gettap / allpass(x, size, fb), the one-pole low-pass maxiFilter::lopass of
// src/maximilian.cpp) as plain per-sample arithmetic, the delay lengths as the constructor computes them, the ring order
// of a voice, the tile rule dattaro.hip's time tiles are built on, and a step-by-step walk of one voice (dt_voice_ref)
// over the same state layout as the kernel.  Only + - * and compares: the same text compiles for the host
// (tests/host_dattaro.cpp), where dt_voice_ref is the checker of the GPU tests.  Compile with contraction off.
//
// What the reference computes.  A ring has D slots and an index i that starts at 0; step: i = (i != D-1) ? i+1 : 0.
//   onetap(x):      o = R[i]; R[i] = x; step; return o
//   gettap(p):      with the index AFTER the step: t = i + p; if (t > D-1) t -= D; return R[t]
//   allpass(x, fb): d = R[i]; s = x + d * fb; o = d + (s * (-fb)); R[i] = s; step; return o
//   lopass(x, c):   y = y + c * (x - y)
// Per sample (sigl, sigr are last sample's):
//   b = lp0(in, 0.8); d = AP1(AP0(AP1(AP0(b, 0.75), 0.75), 0.625), 0.625)   -- serialallpass ignores `firstfilter`: the second
//                                                                              pair runs on rings AP0, AP1 AGAIN (two steps a
//                                                                              sample); fbap[2], fbap[3] are never touched
//   l = d + 0.3 * sigr; r = d + 0.3 * sigl
//   l = AP4(l, 0.7); l = D0.onetap(l); taps 0 1 11 of D0; l = lp1(l, 0.4); l = AP5(l, 0.5); taps 2 12 of AP5's ring;
//   l = D1.onetap(l); taps 3 13 of D1;      the right side the same over AP6, D2 (taps 4 7 8), lp2, AP7 (5 9), D3 (6 10)
//   sigl = l; sigr = r
//   out[0] = t0 + t1 - t2 + t3 - t4 - t5 - t6; out[1] = t7 + t8 - t9 + t10 - t11 - t12 - t13     (left to right)
// The constructor fixes every length from maxiSettings::sampleRate in float arithmetic (dt_scale).  The 3 100-slot
// pre-delay ring (maxiDelays[4]) is private and its output is used by nothing: no call can observe it, and the bank
// does not carry it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"

namespace mxg {
namespace {

constexpr int DT_RINGS = 10, DT_TAPS = 14, DT_STATE = 5;  // = MXG_DATTARO_RINGS / _TAPS / _STATE
constexpr int DT_MAX_LEN = 44100;                         // the reference's ring size
// ---- ring order inside a voice's ring area: the two input allpasses, the four tank allpasses, the four delays ---------
constexpr int DT_AP0 = 0, DT_AP1 = 1, DT_AP4 = 2, DT_AP5 = 3, DT_AP6 = 4, DT_AP7 = 5, DT_D0 = 6, DT_D1 = 7, DT_D2 = 8, DT_D3 = 9;
// state [V][5]
constexpr int DT_LP0 = 0, DT_LP1 = 1, DT_LP2 = 2, DT_SIGL = 3, DT_SIGR = 4;

// lengths at 29.8 kHz (fbap[0], [1], [4..7]; dattarofixdellengths[0..3]) and the tap positions there
MXG_HD constexpr int dt_orig_len(int r) {
    return r == 0 ? 142 : r == 1 ? 107 : r == 2 ? 908 : r == 3 ? 2656 : r == 4 ? 672 : r == 5 ? 1800 : r == 6 ? 4217
           : r == 7 ? 3163 : r == 8 ? 4453 : 3720;
}
MXG_HD constexpr int dt_orig_tap(int j) {
    return j == 0 ? 266 : j == 1 ? 2974 : j == 2 ? 1913 : j == 3 ? 1996 : j == 4 ? 1990 : j == 5 ? 187 : j == 6 ? 1066
           : j == 7 ? 353 : j == 8 ? 3627 : j == 9 ? 1228 : j == 10 ? 2673 : j == 11 ? 2111 : j == 12 ? 335 : 121;
}
// the ring tap j reads
MXG_HD constexpr int dt_tap_ring(int j) {
    return (j == 0 || j == 1 || j == 11) ? DT_D0 : (j == 2 || j == 12) ? DT_AP5 : (j == 3 || j == 13) ? DT_D1
           : (j == 4 || j == 7 || j == 8) ? DT_D2 : (j == 5 || j == 9) ? DT_AP7 : DT_D3;
}
MXG_HD constexpr int dt_steps(int r) { return r < 2 ? 2 : 1; }  // steps per sample

// the constructor's float arithmetic: floor(((float)orig / 29.8f) * ((float)sampleRate / 1000.0f))
static inline int dt_scale(int orig, uint32_t sample_rate) {
    const float dms = 29.8f;
    const float cms = (float)sample_rate / 1000.0f;
    const float prev = (float)orig / dms;
    return (int)floor(prev * cms);
}

struct DtLayout {
    int len[DT_RINGS], off[DT_RINGS], tap[DT_TAPS];
    int S;  // ring doubles per voice
};

static inline DtLayout dt_layout(uint32_t sample_rate) {
    DtLayout L;
    int o = 0;
    for (int r = 0; r < DT_RINGS; r++) {
        L.len[r] = dt_scale(dt_orig_len(r), sample_rate);
        L.off[r] = o;
        o += L.len[r] > 0 ? L.len[r] : 0;
    }
    L.S = o;
    for (int j = 0; j < DT_TAPS; j++) L.tap[j] = dt_scale(dt_orig_tap(j), sample_rate);
    return L;
}

// ---- the tile rule -------------------------------------------------------------------------------------------------
// L samples in one parallel pass over a ring of D slots stepped `steps` times a sample touch steps*L distinct slots iff
// steps*L <= D.  A tap at position p reads what was written D-1-p samples earlier: the sample's own write (distance 0),
// or, when the distance is at least L, something older than the tile -- provided every tap read of the tile comes before
// any of its writes, because the slot may be overwritten later in the same tile.
MXG_HD constexpr bool dt_tile_ok_ring(int D, int steps, int T) { return steps * T <= D; }
MXG_HD constexpr int dt_tap_dist(int D, int p) { return D - 1 - p; }
MXG_HD constexpr bool dt_tile_ok_tap(int D, int p, int T) { return dt_tap_dist(D, p) == 0 || dt_tap_dist(D, p) >= T; }
// A sample rate is accepted iff every length lies in [2, DT_MAX_LEN] and a tile of T samples is legal on the eight tank
// rings and on all fourteen taps.  (The two input rings are walked in sub-tiles where they are shorter than 2*T.)
static inline bool dt_accepts(const DtLayout &L, int T) {
    for (int r = 0; r < DT_RINGS; r++) {
        if (L.len[r] < 2 || L.len[r] > DT_MAX_LEN) return false;
        if (r >= 2 && !dt_tile_ok_ring(L.len[r], 1, T)) return false;
    }
    for (int j = 0; j < DT_TAPS; j++)
        if (!dt_tile_ok_tap(L.len[dt_tap_ring(j)], L.tap[j], T)) return false;
    return true;
}
// samples per parallel pass over the two doubly stepped input rings
MXG_HD int dt_in_sub_len(int D0, int D1, int T) {
    const int D = D0 < D1 ? D0 : D1;
    return D / 2 < T ? D / 2 : T;
}

// ---- the per-sample arithmetic -----------------------------------------------------------------------------------
MXG_HD double dt_lopass(double y, double c, double x) { return y + c * (x - y); }
// one allpass step: `t` comes in as the stage's input and leaves as its output; returns what the ring slot gets
MXG_HD double dt_allpass(double d, double &t, double fb) {
    const double s = t + d * fb;
    t = d + (s * (-fb));
    return s;
}
MXG_HD double dt_cross(double d, double sig) { return d + 0.3 * sig; }
MXG_HD double dt_mix(double a, double b, double c, double d, double e, double f, double g) { return a + b - c + d - e - f - g; }

// ---- slot arithmetic ---------------------------------------------------------------------------------------------
// A stored index outside its ring restarts at slot 0 (the reference cannot produce one).
MXG_HD int dt_idx_fix(int32_t idx, int D) { return (uint32_t)idx < (uint32_t)D ? idx : 0; }
// the slot of the k-th step after `idx`, 0 <= k <= D
MXG_HD int dt_slot(int idx, int k, int D) {
    const int s = idx + k;
    return s >= D ? s - D : s;
}
// the slot gettap(p) reads after the k-th step after `idx` has been taken (k steps done, index at idx + k + 1), 0 <= k < D
MXG_HD int dt_tap_slot(int idx, int k, int p, int D) {
    int s = idx + k + 1 + p;
    if (s >= D) s -= D;
    if (s >= D) s -= D;
    return s;
}
MXG_HD int dt_idx_after(int idx, int k, int D) { return (idx + k) % D; }

// ---- one voice, one sample at a time, over the bank's state layout ---------------------------------------------------
// rings [V][S] (voice-major, ring r at L.off[r]), idx int32 [V][10], state [V][5] = lp0 lp1 lp2 sigl sigr.
// in [N][V]; out [2][N][V].
struct DtArgs {
    size_t V, N;
    const double *in;
    double *rings;
    int32_t *idx;
    double *state;
    double *out;
    DtLayout L;
};

static inline void dt_voice_ref(const DtArgs &A, size_t v) {
    const size_t V = A.V, N = A.N;
    const DtLayout &L = A.L;
    double *ring = A.rings + v * (size_t)L.S;
    int idx[DT_RINGS];
    for (int r = 0; r < DT_RINGS; r++) idx[r] = dt_idx_fix(A.idx[v * DT_RINGS + r], L.len[r]);
    double *st = A.state + v * DT_STATE;
    double y0 = st[DT_LP0], y1 = st[DT_LP1], y2 = st[DT_LP2], sigl = st[DT_SIGL], sigr = st[DT_SIGR];
    auto step = [&](int r) { idx[r] = idx[r] != L.len[r] - 1 ? idx[r] + 1 : 0; };
    auto allpass = [&](int r, double x, double fb) {
        double *slot = ring + L.off[r] + idx[r];
        *slot = dt_allpass(*slot, x, fb);
        step(r);
        return x;
    };
    auto onetap = [&](int r, double x) {
        double *slot = ring + L.off[r] + idx[r];
        const double o = *slot;
        *slot = x;
        step(r);
        return o;
    };
    auto gettap = [&](int j) {
        const int r = dt_tap_ring(j);
        int t = idx[r] + L.tap[j];
        if (t > L.len[r] - 1) t -= L.len[r];
        return ring[L.off[r] + t];
    };
    for (size_t n = 0; n < N; n++) {
        y0 = dt_lopass(y0, 0.8, A.in[n * V + v]);
        double d = allpass(DT_AP0, y0, 0.75);
        d = allpass(DT_AP1, d, 0.75);
        d = allpass(DT_AP0, d, 0.625);
        d = allpass(DT_AP1, d, 0.625);
        double l = dt_cross(d, sigr), r = dt_cross(d, sigl);
        double t[DT_TAPS];
        l = allpass(DT_AP4, l, 0.7);
        l = onetap(DT_D0, l);
        t[0] = gettap(0), t[1] = gettap(1), t[11] = gettap(11);
        y1 = dt_lopass(y1, 0.4, l);
        l = allpass(DT_AP5, y1, 0.5);
        t[2] = gettap(2), t[12] = gettap(12);
        l = onetap(DT_D1, l);
        t[3] = gettap(3), t[13] = gettap(13);
        r = allpass(DT_AP6, r, 0.7);
        r = onetap(DT_D2, r);
        t[4] = gettap(4), t[7] = gettap(7), t[8] = gettap(8);
        y2 = dt_lopass(y2, 0.4, r);
        r = allpass(DT_AP7, y2, 0.5);
        t[5] = gettap(5), t[9] = gettap(9);
        r = onetap(DT_D3, r);
        t[6] = gettap(6), t[10] = gettap(10);
        sigl = l;
        sigr = r;
        A.out[n * V + v] = dt_mix(t[0], t[1], t[2], t[3], t[4], t[5], t[6]);
        A.out[(N + n) * V + v] = dt_mix(t[7], t[8], t[9], t[10], t[11], t[12], t[13]);
    }
    for (int r = 0; r < DT_RINGS; r++) A.idx[v * DT_RINGS + r] = idx[r];
    st[DT_LP0] = y0, st[DT_LP1] = y1, st[DT_LP2] = y2, st[DT_SIGL] = sigl, st[DT_SIGR] = sigr;
}

}  // namespace
}  // namespace mxg
