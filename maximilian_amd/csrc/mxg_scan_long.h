// mxg_scan_long.h -- the arithmetic of the LONG time-parallel scan (scan_long.hip, K28; mxg_scan_long_render / _host): few voices,
// blocks of any length.  It is K10's scan (mxg_scan.h) one level up, over the same lane-exchange primitive, so that the same text
// runs on a wavefront (scan_long.hip) and on the host (scan_long_host.cpp, tests/host_scan_long_main.cpp).  Only + - * in a fixed
// order, contraction off: the device must give the host twin's bits (tests/test_gpu_scan_long.py).
//
// Kinds 0-4 are mxg_scan.h's; kind 5 is maxiLagExp<double>::addSample (H:523-556), val = (alpha * x) + (alphaReciprocal * val),
// one state double, coefficient rows alpha, alphaReciprocal.
//
// The decomposition of a call of N samples per voice, a function of N alone (T = kLongChunk = 2048 = 64 lanes x L = 32):
//   C = N / T whole chunks, then the remainder R = N % T as at most five K10 blocks of 64 * 2^j samples, j = 4, 3, 2, 1, 0, one for
//   every set bit of R / 64 from the highest down (L = 2^j), then R % 64 plain steps.  Every piece is rendered by the reference's own
//   step from a start state; what differs from the sequential recurrence is only how the start states of the chunks and of the
//   lanes inside a block are reached.
// Three phases (three launches on the device, each finished before the next starts):
//   A. for the chunks c = 0 .. C-2: e_c = the state chunk c's inputs alone leave from the ZERO state, in the scan's basis
//      (scan_voice's steps 1-3, lane 63's scanned value: scan_summary).  Chunk 0 starts from the carried-in state instead, so e_0 is
//      the true state after chunk 0.  (The last chunk's summary is needed by nobody.)
//   B. one executor per voice: E_c = the true state after chunk c, E_0 = e_0, E_c = M_T E_{c-1} + e_c, where M_T is the T-step
//      transition: K10's M (L = 32 steps, from the unit states, the step a black box) squared six times (scan_chunk_transition).
//      scan_chunks: lane k owns the run of r = ceil((C-1) / 64) consecutive chunks [k r, (k+1) r), composes them serially from zero,
//      M_r = M_T^r comes from the unit states through r applications of M_T, a Kogge-Stone over the lanes with M_r^(2^j), and the
//      lane walks its run again from the scanned state of the lane below and writes every E_c.  scan_voice's shape, one level up.
//   C. every chunk c runs the whole of scan_voice from its start state (c = 0: the carried-in state; else scan_restart(E_{c-1})) and
//      writes its outputs; the executor of the last chunk goes on through the remainder (scan_tail) and writes the carried state.
// A call with C <= 1 is phase C alone, and a call of N = 64 * 2^j <= 2048 is one K10 block: K10's bits.
//
// Non-finite input: a NaN or Inf sample makes every later output and state of its voice non-finite where the sequential recurrence's
// are (0 * Inf = NaN and x * NaN = NaN keep a bad E_c bad through every product), but WHICH of NaN and Inf may differ: entries of
// M_T underflow to 0 for fast-decaying settings, and 0 * Inf is NaN where the sequential recurrence still holds Inf.
#pragma once
#include <stddef.h>

#include "mxg_hd.h"
#include "mxg_scan.h"

namespace mxg {
namespace {

constexpr int kLongChunk = kScanLanes * kScanMaxL;  // T = 2048
constexpr int kLongKinds = 6;
constexpr int scan_long_ncoef(int kind) { return kind == 5 ? 2 : scan_ncoef(kind); }   // coefficient rows [NC][V]
constexpr int scan_long_nstate(int kind) { return kind == 5 ? 1 : scan_nstate(kind); }  // state rows read and written

// maxiLagExp<double>::addSample, verbatim from mxg_classic.h's cls_lag: a = val; c[0] = alpha, c[1] = alphaReciprocal
template <>
struct ScanStep<5> {
    double c[9];
    MXG_HD double operator()(S3 &s, double x) const {
        s.a = (c[0] * x) + (c[1] * s.a);
        return s.a;
    }
};

MXG_HD S3 scan_add(const S3 &p, const S3 &q) { return S3{p.a + q.a, p.b + q.b, p.c + q.c}; }

// K10's M (the L-step transition with zero input in the scan's basis, from the unit states of lanes 0..2) for L = 32, squared six
// times: the transition over one chunk of 64 * 32 samples.  The same in every slot.
template <int KIND, int W, class X>
MXG_HD M3 scan_chunk_transition(const X &xch, const ScanStep<KIND> &step) {
    double ua[W], ub[W], uc[W];
    for (int w = 0; w < W; w++) {
        const int lane = xch.lane(w);
        S3 u = scan_unit_state<KIND>(S3{lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0});
        for (int i = 0; i < kScanMaxL; i++) (void)step(u, 0.0);
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
    for (int d = 1; d < kScanLanes; d <<= 1) M = square(M);
    return M;
}

// Phase A: scan_voice's steps 1-3 over one block of 64 * L samples -- lane 63's scanned value, the state after the block in the
// scan's basis (from s_in where `first`, else from the zero state).  The same in every slot.
template <int KIND, int L, int W, class X>
MXG_HD S3 scan_summary(const X &xch, const ScanStep<KIND> &step, bool first, const S3 &s_in, const double (&x)[W][L]) {
    double qa[W], qb[W], qc[W], ua[W], ub[W], uc[W];
    for (int w = 0; w < W; w++) {
        const int lane = xch.lane(w);
        S3 q = (lane == 0 && first) ? s_in : S3{0.0, 0.0, 0.0};
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
    return S3{xch.from(qa, kScanLanes - 1), xch.from(qb, kScanLanes - 1), xch.from(qc, kScanLanes - 1)};
}

// Phase B, one voice: the K summaries e_0 .. e_{K-1} (get_e(c)) -> the true states E_0 .. E_{K-1} after those chunks (put_E(c, E)),
// E_0 = e_0, E_c = MT E_{c-1} + e_c.  Lane k owns the chunks [k r, (k+1) r) below K, r = ceil(K / 64); the lanes past the last chunk
// own nothing and nobody reads them.
template <int W, class X, class GE, class PE>
MXG_HD void scan_chunks(const X &xch, const M3 &MT, size_t K, GE &&get_e, PE &&put_E) {
    const size_t r = (K + kScanLanes - 1) / kScanLanes;
    double qa[W], qb[W], qc[W], ua[W], ub[W], uc[W];
    for (int w = 0; w < W; w++) {
        const size_t lo = (size_t)xch.lane(w) * r, hi = lo + r < K ? lo + r : K;
        S3 q = {0.0, 0.0, 0.0};
        for (size_t c = lo; c < hi; c++) q = c == lo ? get_e(c) : scan_add(apply(MT, q), get_e(c));
        qa[w] = q.a, qb[w] = q.b, qc[w] = q.c;
        const int lane = xch.lane(w);
        S3 u = {lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0};
        for (size_t i = 0; i < r; i++) u = apply(MT, u);
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
        const size_t lo = (size_t)xch.lane(w) * r, hi = lo + r < K ? lo + r : K;
        S3 s = {sa[w], sb[w], sc[w]};
        for (size_t c = lo; c < hi; c++) {
            s = c == 0 ? get_e(c) : scan_add(apply(MT, s), get_e(c));
            put_E(c, s);
        }
    }
}

// One K10 block of 64 * L samples from the state s: ld(w, n) is sample n of the block for slot w, st(w, n, y) takes output n.
// Every input is loaded before the first output leaves.  Returns the state after the block, the same in every slot.
template <int KIND, int L, int W, class X, class LD, class ST>
MXG_HD S3 scan_block(const X &xch, const ScanStep<KIND> &step, const S3 &s, LD &&ld, ST &&st) {
    double x[W][L];
    for (int w = 0; w < W; w++) {
        MXG_SCAN_UNROLL
        for (int i = 0; i < L; i++) x[w][i] = ld(w, (size_t)xch.lane(w) * L + i);
    }
    S3 e[W];
    scan_voice<KIND, L, W>(xch, step, s, x, [&](int w, int i, double y) { st(w, (size_t)xch.lane(w) * L + i, y); }, e);
    double ea[W], eb[W], ec[W];
    for (int w = 0; w < W; w++) ea[w] = e[w].a, eb[w] = e[w].b, ec[w] = e[w].c;
    return S3{xch.from(ea, kScanLanes - 1), xch.from(eb, kScanLanes - 1), xch.from(ec, kScanLanes - 1)};
}

// The remainder of a voice, R < 2048 samples from the state s: K10 blocks for the set bits of R / 64 from the highest down, then
// R % 64 plain steps (ld1(n) / st1(n, y): once per executor).  n counts from the remainder's first sample.  Returns the state after it.
template <int KIND, int W, class X, class LD, class ST, class LD1, class ST1>
MXG_HD S3 scan_tail(const X &xch, const ScanStep<KIND> &step, S3 s, size_t R, LD &&ld, ST &&st, LD1 &&ld1, ST1 &&st1) {
    size_t at = 0;
    auto ldo = [&](int w, size_t n) { return ld(w, at + n); };
    auto sto = [&](int w, size_t n, double y) { st(w, at + n, y); };
    if (R & 1024) s = scan_block<KIND, 16, W>(xch, step, s, ldo, sto), at += 1024;
    if (R & 512) s = scan_block<KIND, 8, W>(xch, step, s, ldo, sto), at += 512;
    if (R & 256) s = scan_block<KIND, 4, W>(xch, step, s, ldo, sto), at += 256;
    if (R & 128) s = scan_block<KIND, 2, W>(xch, step, s, ldo, sto), at += 128;
    if (R & 64) s = scan_block<KIND, 1, W>(xch, step, s, ldo, sto), at += 64;
    for (; at < R; at++) st1(at, step(s, ld1(at)));
    return s;
}

// ---- the host twin: the three phases over arrays of 64 lane values (plain C++ translation units only) -------------------------
#if !defined(__HIPCC__)
struct LongHostXch {
    int lane(int w) const { return w; }
    void up(const double (&src)[kScanLanes], int d, double (&dst)[kScanLanes]) const {
        for (int k = 0; k < kScanLanes; k++) dst[k] = k >= d ? src[k - d] : src[k];
    }
    double from(const double (&src)[kScanLanes], int j) const { return src[j]; }
};

// in / out [N][V] (out == in allowed), coef [NC][V], st [NS][V]; work: 3 * (C - 1) doubles for one voice's E (C = N / 2048), or null if C <= 1
template <int KIND>
inline void scan_long_host_voices(size_t V, size_t N, const double *in, const double *coef, double *st, double *out, double *work) {
    constexpr int NC = scan_long_ncoef(KIND), NS = scan_long_nstate(KIND), W = kScanLanes, L = kScanMaxL;
    const size_t T = kLongChunk, C = N / T, K = C > 1 ? C - 1 : 0, R = N % T;
    const LongHostXch xch;
    for (size_t v = 0; v < V; v++) {
        ScanStep<KIND> step;
        for (int r = 0; r < 9; r++) step.c[r] = r < NC ? coef[(size_t)r * V + v] : 0.0;
        S3 s = {st[v], NS >= 2 ? st[V + v] : 0.0, NS == 3 ? st[2 * V + v] : 0.0};
        const S3 s_in = s;
        double x[W][L];
        for (size_t c = 0; c < K; c++) {  // A
            for (int k = 0; k < W; k++)
                for (int i = 0; i < L; i++) x[k][i] = in[(c * T + (size_t)k * L + i) * V + v];
            const S3 e = scan_summary<KIND, L, W>(xch, step, c == 0, s_in, x);
            work[3 * c] = e.a, work[3 * c + 1] = e.b, work[3 * c + 2] = e.c;
        }
        if (K) {  // B: the summaries work[0 .. 3K) -> the states work[3K .. 6K)
            const M3 MT = scan_chunk_transition<KIND, W>(xch, step);
            double *E = work, *E2 = work + 3 * K;
            scan_chunks<W>(xch, MT, K, [&](size_t c) { return S3{E[3 * c], E[3 * c + 1], E[3 * c + 2]}; },
                           [&](size_t c, const S3 &q) { E2[3 * c] = q.a, E2[3 * c + 1] = q.b, E2[3 * c + 2] = q.c; });
        }
        for (size_t c = 0; c < C; c++) {  // C
            if (c) s = scan_restart<KIND>(S3{work[3 * (K + c - 1)], work[3 * (K + c - 1) + 1], work[3 * (K + c - 1) + 2]});
            const size_t n0 = c * T;
            s = scan_block<KIND, L, W>(xch, step, s, [&](int, size_t n) { return in[(n0 + n) * V + v]; },
                                       [&](int, size_t n, double y) { out[(n0 + n) * V + v] = y; });
        }
        const size_t n0 = C * T;
        s = scan_tail<KIND, W>(xch, step, s, R, [&](int, size_t n) { return in[(n0 + n) * V + v]; },
                               [&](int, size_t n, double y) { out[(n0 + n) * V + v] = y; },
                               [&](size_t n) { return in[(n0 + n) * V + v]; }, [&](size_t n, double y) { out[(n0 + n) * V + v] = y; });
        st[v] = s.a;
        if (NS >= 2) st[V + v] = s.b;
        if (NS == 3) st[2 * V + v] = s.c;
    }
}

// work: 6 * (N / 2048) doubles (summaries and states of one voice), may be null when N < 2 * 2048.  Returns 0, or 1 for an unknown kind.
inline int scan_long_host_run(int kind, size_t V, size_t N, const double *in, const double *coef, double *st, double *out, double *work) {
    switch (kind) {
        case 0: scan_long_host_voices<0>(V, N, in, coef, st, out, work); return 0;
        case 1: scan_long_host_voices<1>(V, N, in, coef, st, out, work); return 0;
        case 2: scan_long_host_voices<2>(V, N, in, coef, st, out, work); return 0;
        case 3: scan_long_host_voices<3>(V, N, in, coef, st, out, work); return 0;
        case 4: scan_long_host_voices<4>(V, N, in, coef, st, out, work); return 0;
        case 5: scan_long_host_voices<5>(V, N, in, coef, st, out, work); return 0;
    }
    return 1;
}
#endif  // !__HIPCC__

}  // namespace
}  // namespace mxg
