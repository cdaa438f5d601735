// mxg_scan.h -- the arithmetic of the time-parallel scan of small linear-filter banks (scan.hip, K10; knob "time_parallel"):
// the five one-sample steps, the 3x3 transition algebra and the per-voice algorithm itself, written over a LANE-EXCHANGE
// primitive so that the same text runs on a wavefront (scan.hip: one lane per executor, shuffles / readlane) and on the host
// (tests/host_scan.cpp: one executor holding all 64 lanes in arrays).  Only + - * in a fixed order, contraction off: the device
// must equal the host build bit for bit (tests/test_gpu_scan.py), even though neither equals the sequential recurrence.
//
// The exchange primitive X over W lane slots per executor (W = 1 on the device, 64 on the host):
//   int    X::lane(w)             the lane number (0..63) of slot w
//   void   X::up(src, d, dst)     dst[w] = src of lane(w) - d          (lanes below d: anything; never used)
//   double X::from(src, j)        src of lane j                          (the same value in every slot)
#pragma once
#include "mxg_hd.h"

#if defined(__HIPCC__)  // (g++ -Wall warns about a pragma it does not know)
#define MXG_SCAN_UNROLL _Pragma("unroll")
#else
#define MXG_SCAN_UNROLL
#endif

namespace mxg {
namespace {

struct S3 {
    double a, b, c;
};

constexpr int kScanLanes = 64;
constexpr int kScanMaxL = 32;
constexpr int scan_ncoef(int kind) { return kind == 0 ? 1 : (kind == 1 ? 9 : (kind == 2 ? 5 : 2)); }  // coefficient rows [NC][V]
constexpr int scan_nstate(int kind) { return kind == 0 || kind >= 3 ? 2 : 3; }                        // state rows read and written

// the one-sample steps, verbatim from filter2.hip / voice.hip (state in s, returns the output)
template <int KIND>
struct ScanStep {
    double c[9];
    MXG_HD double operator()(S3 &s, double x) const {
        if constexpr (KIND == 0) {  // maxiDCBlocker: a = xm1, b = ym1
            s.b = x - s.a + c[0] * s.b;
            s.a = x;
            return s.b;
        } else if constexpr (KIND == 1) {  // maxiSVF: a = v0z, b = v1, c = v2
            const double v1z = s.b, v2z = s.c;
            const double v3 = x + s.a - 2.0 * v2z;
            s.b += c[0] * v3 - c[1] * v1z;
            s.c += c[2] * v3 + c[3] * v1z;
            s.a = x;
            const double low = s.c, band = s.b;
            const double high = x - c[4] * s.b - s.c;
            const double notch = x - c[4] * s.b;
            return (low * c[5]) + (band * c[6]) + (high * c[7]) + (notch * c[8]);
        } else if constexpr (KIND == 2) {  // maxiBiquad, direct form II: a = v[0], b = v[1], c = v[2]
            s.a = x - (c[3] * s.b) - (c[4] * s.c);
            const double o = (c[0] * s.a) + (c[1] * s.b) + (c[2] * s.c);
            s.c = s.b;
            s.b = s.a;
            return o;
        } else {  // maxiFilter::lores (3) / hires (4): a = x, b = y; c[0] = c, c[1] = r
            s.a = s.a + (x - s.b) * c[0];
            s.b = s.b + s.a;
            s.a = s.a * c[1];
            return KIND == 3 ? s.b : x - s.b;
        }
    }
};

struct M3 {
    double m[3][3];  // m[i][j]: coefficient of state j in new state i
};
MXG_HD S3 apply(const M3 &M, const S3 &v) {
    S3 r;
    r.a = M.m[0][0] * v.a + M.m[0][1] * v.b + M.m[0][2] * v.c;
    r.b = M.m[1][0] * v.a + M.m[1][1] * v.b + M.m[1][2] * v.c;
    r.c = M.m[2][0] * v.a + M.m[2][1] * v.b + M.m[2][2] * v.c;
    return r;
}
MXG_HD M3 square(const M3 &A) {
    M3 R;
    MXG_SCAN_UNROLL
    for (int i = 0; i < 3; i++)
        MXG_SCAN_UNROLL
        for (int j = 0; j < 3; j++) R.m[i][j] = A.m[i][0] * A.m[0][j] + A.m[i][1] * A.m[1][j] + A.m[i][2] * A.m[2][j];
    return R;
}
// A * B over the leading D x D block (D = 3: the general product; the entries outside the block are neither read nor written)
template <int D = 3>
MXG_HD M3 product(const M3 &A, const M3 &B) {
    M3 R = {};
    MXG_SCAN_UNROLL
    for (int i = 0; i < D; i++)
        MXG_SCAN_UNROLL
        for (int j = 0; j < D; j++) {
            double t = A.m[i][0] * B.m[0][j];
            MXG_SCAN_UNROLL
            for (int k = 1; k < D; k++) t = t + A.m[i][k] * B.m[k][j];
            R.m[i][j] = t;
        }
    return R;
}

// The basis the scan is carried in.  maxiBiquad with both poles near z = 1 (a 20 ... 60 Hz cutoff): the direct-form-II states reach
// ~1 / (1 + b1 + b2) times the input (1e5 at 20 Hz) with v1 ~ v2, and the entries of A^n grow like n, so M * (v0, v1, v2) forms
// differences like (n + 1) v1 - n v2 of terms near 1e9 whose result is near 1e5: 1e-8 x peak at N = 2048.  So the biquad's scan
// takes its state as (v1, d = v1 - v2): the unit-state recurrences start from v1 = v2 = 1 and from v2 = -1, and the products stay
// near the size of their result.  It is carried as w = (v2, v1, d): v0 is never read by the step (it is written first), its slot
// takes v2, which the restart then reads as it is -- v1 - d would be Inf - Inf after an infinite sample that ends a segment, where
// the sequential recurrence still has a finite v2.  Column 0 of M is zero.  d = v1 - v2 of two near-equal doubles is exact or
// nearly so.  The other kinds are carried as they are.
template <int KIND>
MXG_HD S3 scan_to_basis(const S3 &s) {  // a state -> what the scan carries
    if constexpr (KIND == 2) return S3{s.c, s.b, s.b - s.c};
    else return s;
}
template <int KIND>
MXG_HD S3 scan_unit_state(const S3 &e) {  // the state whose carried form is the unit vector e (as far as the scan reads it)
    if constexpr (KIND == 2) return S3{0.0, e.b, e.b - e.c};
    else return e;
}
template <int KIND>
MXG_HD S3 scan_restart(const S3 &w) {  // what the scan carries -> the state a segment starts from
    if constexpr (KIND == 2) return S3{w.b, w.b, w.a};
    else return w;
}

// One voice, one block of 64 * L samples: lane k owns the samples [kL, (k+1)L), x[w][i] = sample lane(w) * L + i.
//   1. every lane runs its segment from the ZERO state (lane 0: from the carried-in state s_in): e_k, taken to the scan's basis;
//   2. M = the L-step transition with zero input in that basis, from the unit states carried by lanes 0..2 (the step is a black box);
//   3. end_k = M end_{k-1} + e_k: Kogge-Stone over the lanes, M <- M * M between the steps;
//   4. lane k restarts from end_{k-1}, taken back from the scan's basis, and renders its samples with the step itself: out(w, i, y); s_end[w] is the state after
//      the lane's last sample (lane 63: the state the next block continues from).
template <int KIND, int L, int W, class X, class O>
MXG_HD void scan_voice(const X &xch, const ScanStep<KIND> &step, const S3 &s_in, const double (&x)[W][L], O &&out, S3 (&s_end)[W]) {
    double qa[W], qb[W], qc[W], ua[W], ub[W], uc[W];
    for (int w = 0; w < W; w++) {
        const int lane = xch.lane(w);
        S3 q = lane == 0 ? s_in : S3{0.0, 0.0, 0.0};
        MXG_SCAN_UNROLL
        for (int i = 0; i < L; i++) (void)step(q, x[w][i]);
        q = scan_to_basis<KIND>(q);
        qa[w] = q.a, qb[w] = q.b, qc[w] = q.c;
        S3 u = scan_unit_state<KIND>(S3{lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0});
        MXG_SCAN_UNROLL
        for (int i = 0; i < L; i++) (void)step(u, 0.0);
        u = scan_to_basis<KIND>(u);
        ua[w] = u.a, ub[w] = u.b, uc[w] = u.c;
    }
    M3 M;
    MXG_SCAN_UNROLL
    for (int j = 0; j < 3; j++) {
        M.m[0][j] = xch.from(ua, j);
        M.m[1][j] = xch.from(ub, j);
        M.m[2][j] = xch.from(uc, j);
    }
    MXG_SCAN_UNROLL
    for (int d = 1; d < kScanLanes; d <<= 1) {
        double pa[W], pb[W], pc[W];
        xch.up(qa, d, pa);
        xch.up(qb, d, pb);
        xch.up(qc, d, pc);
        for (int w = 0; w < W; w++)
            if (xch.lane(w) >= d) {
                const S3 t = apply(M, S3{pa[w], pb[w], pc[w]});
                qa[w] += t.a;
                qb[w] += t.b;
                qc[w] += t.c;
            }
        if (d < kScanLanes / 2) M = square(M);
    }
    double sa[W], sb[W], sc[W];
    xch.up(qa, 1, sa);
    xch.up(qb, 1, sb);
    xch.up(qc, 1, sc);
    for (int w = 0; w < W; w++) {
        S3 s = scan_restart<KIND>(S3{sa[w], sb[w], sc[w]});
        if (xch.lane(w) == 0) s = s_in;
        MXG_SCAN_UNROLL
        for (int i = 0; i < L; i++) out(w, i, step(s, x[w][i]));
        s_end[w] = s;
    }
}

}  // namespace
}  // namespace mxg
