// mxg_scan_long_swept.h -- the arithmetic of the long time-parallel scan with PER-SAMPLE coefficients (scan_long_swept.hip, K31;
// mxg_scan_long_render_swept / mxg_scan_long_swept_host): K28 (mxg_scan_long.h) for a filter whose cutoff moves.  Written over the
// lane-exchange primitive of mxg_scan.h, so that the same text runs on a wavefront (scan_long_swept.hip) and on the host
// (scan_long_swept_host.cpp, tests/host_scan_long_swept_main.cpp).  Only + - * in a fixed order, contraction off: the device must give
// the host twin's bits (tests/test_gpu_scan_long_swept.py).
//
// Kinds 3 lores, 4 hires (state (x, y), D = 2) and 5 maxiLagExp (state val, D = 1), the steps ScanStep<3>, <4>, <5> as black boxes,
// called with c[0], c[1] = rows 0, 1 of the coefficients OF THE SAMPLE they process (c, r or alpha, alphaReciprocal).  These kinds'
// states are carried as they are (scan_to_basis is the identity for them).
//
// A time-varying linear recurrence is a scan over affine pairs (M, e), standing for s -> M s + e; the pair of a later piece composed
// with the pair of the piece before it: (M2, e2) o (M1, e1) = (M2 M1, M2 e1 + e2)  (swept_compose; product<D>, then apply then +).
// Where K28 has one M per voice and its powers, every lane and every chunk here has an M of its own.
//
// One block of 64 * L samples from the state s (swept_block; lane k owns the samples [k L, (k + 1) L)):
//   1. e_k: the lane's segment run from the ZERO state (lane 0: from s); M_k: the lane's own L-step transition, column j = the unit
//      state j run through the same L steps -- the lane's own coefficients -- with zero input  (swept_lanes; one loop, D + 1 recurrences);
//   2. an inclusive Kogge-Stone over the lanes, d = 1, 2, 4, 8, 16, 32: lane k >= d takes P_k <- P_k o P_{k-d}, i.e.
//      e_k <- M_k e_{k-d} + e_k (with the M_k from BEFORE this step), then M_k <- M_k M_{k-d}; lanes below d keep theirs  (swept_pair_scan).
//      The association is that of the Kogge-Stone tree: after step d, P_k covers the lanes max(0, k - 2d + 1) .. k;
//   3. lane k restarts from the scanned e_{k-1} (lane 0: from s) and renders its samples with the step itself.
//      The state after the block is lane 63's after its last sample.
//
// The decomposition of a call of N samples per voice, a function of N alone (Ts = kSweptChunk = 1024 = 64 lanes x L = 16):
//   C = N / Ts whole chunks, then the remainder R = N % Ts as at most four blocks of 64 * 2^j samples, j = 3, 2, 1, 0, one for every
//   set bit of R / 64 from the highest down (L = 2^j), then R % 64 plain steps.  A call with N < 64 is plain steps only: the
//   sequential recurrence's bits.
// Three phases (three launches on the device, each finished before the next starts):
//   A. for the chunks c = 0 .. C-2: the chunk's pair P_c = lane 63's inclusive composite of steps 1-2, lane 0 started from zero
//      (swept_summary).  Chunk 0 starts from the carried-in state instead: its e is the true state after it and its M is never read.
//   B. one executor per voice: E_c = the true state after chunk c, E_0 = e_0, E_c = M_c E_{c-1} + e_c  (swept_chunks).  Lane k owns the
//      run of r = ceil((C-1) / 64) consecutive chunks [k r, (k+1) r) and folds their pairs from the left, ((P_lo+1 o P_lo) o ...); a lane
//      whose run is empty holds the identity.  The Kogge-Stone of step 2 over the lanes on the run pairs; then every lane walks its
//      run again from the scanned state of the lane below and writes E_c after every chunk.
//   C. every chunk c is one swept_block from its start state (c = 0: the carried-in state; else E_{c-1}); the executor of the last chunk
//      goes on through the remainder (swept_tail) and writes the rows of the state the kind owns.
// A call with C <= 1 is phase C alone.
//
// Non-finite input: as K28 -- a NaN or Inf sample makes every later output and state of its voice non-finite where the sequential
// recurrence's are (x * NaN = NaN and 0 * Inf = NaN keep a bad e bad through every product), but WHICH of NaN and Inf may differ.
// Other voices are separate executors and keep their bits.
#pragma once
#include <stddef.h>

#include "mxg_hd.h"
#include "mxg_scan.h"
#include "mxg_scan_long.h"

namespace mxg {
namespace {

constexpr int kSweptL = 16;
constexpr int kSweptChunk = kScanLanes * kSweptL;  // Ts = 1024
constexpr int kSweptMinRows = 2, kSweptMaxRows = 8;
constexpr bool swept_kind(int kind) { return kind >= 3 && kind <= 5; }
constexpr int swept_dim(int kind) { return kind == 5 ? 1 : 2; }  // D: the state doubles the step reads and writes

struct SweptPair {  // s -> M s + e, the leading D x D block of M and the first D entries of e
    M3 M;
    S3 e;
};
constexpr int kSweptPairDoubles = 6;  // a pair in memory: m00 m01 m10 m11 e0 e1 (D = 1: m00 and e0 are read)
constexpr int kSweptEndDoubles = 2;   // a state in memory: a, b

template <int D>
MXG_HD S3 swept_apply(const M3 &M, const S3 &v) {  // apply() over the leading block
    S3 r = {0.0, 0.0, 0.0};
    if constexpr (D == 1) r.a = M.m[0][0] * v.a;
    else if constexpr (D == 2) r.a = M.m[0][0] * v.a + M.m[0][1] * v.b, r.b = M.m[1][0] * v.a + M.m[1][1] * v.b;
    else r = apply(M, v);
    return r;
}
// `hi` after `lo`: (M_hi M_lo, M_hi e_lo + e_hi)
template <int D>
MXG_HD SweptPair swept_compose(const SweptPair &hi, const SweptPair &lo) {
    SweptPair p;
    p.e = scan_add(swept_apply<D>(hi.M, lo.e), hi.e);
    p.M = product<D>(hi.M, lo.M);
    return p;
}
template <int D>
MXG_HD SweptPair swept_identity() {
    SweptPair p = {};
    for (int i = 0; i < D; i++) p.M.m[i][i] = 1.0;
    return p;
}

template <int D, int W>
struct SweptLanes {  // one pair per lane slot, entry by entry (what the exchange primitive moves)
    double e[D][W], m[D * D][W];
    MXG_HD SweptPair get(int w) const {
        SweptPair p = {};
        for (int i = 0; i < D; i++) {
            (i == 0 ? p.e.a : p.e.b) = e[i][w];
            for (int j = 0; j < D; j++) p.M.m[i][j] = m[i * D + j][w];
        }
        return p;
    }
    MXG_HD void put(int w, const SweptPair &p) {
        for (int i = 0; i < D; i++) {
            e[i][w] = i == 0 ? p.e.a : p.e.b;
            for (int j = 0; j < D; j++) m[i * D + j][w] = p.M.m[i][j];
        }
    }
    template <class X>
    MXG_HD SweptPair from(const X &xch, int lane) const {  // lane's pair, the same in every slot
        SweptPair p = {};
        for (int i = 0; i < D; i++) {
            (i == 0 ? p.e.a : p.e.b) = xch.from(e[i], lane);
            for (int j = 0; j < D; j++) p.M.m[i][j] = xch.from(m[i * D + j], lane);
        }
        return p;
    }
};

// Step 1.  ld(w, n): sample n of the block for slot w; cf(w, n, r): row r (0, 1) of that sample's coefficients.
template <int KIND, int L, int W, class X, class LD, class CF>
MXG_HD void swept_lanes(const X &xch, const S3 &s0, LD &&ld, CF &&cf, SweptLanes<swept_dim(KIND), W> &P) {
    constexpr int D = swept_dim(KIND);
    for (int w = 0; w < W; w++) {
        const int lane = xch.lane(w);
        const size_t n0 = (size_t)lane * L;
        ScanStep<KIND> step = {};
        S3 q = lane == 0 ? s0 : S3{0.0, 0.0, 0.0};
        S3 u0 = {1.0, 0.0, 0.0}, u1 = {0.0, 1.0, 0.0};
        MXG_SCAN_UNROLL
        for (int i = 0; i < L; i++) {
            step.c[0] = cf(w, n0 + i, 0);
            step.c[1] = cf(w, n0 + i, 1);
            (void)step(q, ld(w, n0 + i));
            (void)step(u0, 0.0);
            if constexpr (D == 2) (void)step(u1, 0.0);
        }
        SweptPair p = {};
        p.e = q;
        p.M.m[0][0] = u0.a;
        if constexpr (D == 2) p.M.m[1][0] = u0.b, p.M.m[0][1] = u1.a, p.M.m[1][1] = u1.b;
        P.put(w, p);
    }
}

// Step 2.  WITH_M = false leaves the last step's product out: after it only e is read (the e are the same bits either way).
template <int D, int W, bool WITH_M, class X>
MXG_HD void swept_pair_scan(const X &xch, SweptLanes<D, W> &P) {
    MXG_SCAN_UNROLL
    for (int d = 1; d < kScanLanes; d <<= 1) {
        SweptLanes<D, W> Q;
        for (int i = 0; i < D; i++) xch.up(P.e[i], d, Q.e[i]);
        for (int i = 0; i < D * D; i++) xch.up(P.m[i], d, Q.m[i]);
        for (int w = 0; w < W; w++)
            if (xch.lane(w) >= d) {
                const SweptPair hi = P.get(w), lo = Q.get(w);
                if (WITH_M || d < kScanLanes / 2) P.put(w, swept_compose<D>(hi, lo));
                else {
                    const S3 e = scan_add(swept_apply<D>(hi.M, lo.e), hi.e);
                    P.e[0][w] = e.a;
                    if constexpr (D == 2) P.e[1][w] = e.b;
                }
            }
    }
}

// Phase A: steps 1-2 over one block, lane 63's inclusive composite; lane 0 starts from s0.  The same in every slot.
template <int KIND, int L, int W, class X, class LD, class CF>
MXG_HD SweptPair swept_summary(const X &xch, const S3 &s0, LD &&ld, CF &&cf) {
    constexpr int D = swept_dim(KIND);
    SweptLanes<D, W> P;
    swept_lanes<KIND, L, W>(xch, s0, ld, cf, P);
    swept_pair_scan<D, W, true>(xch, P);
    return P.from(xch, kScanLanes - 1);
}

// One block of 64 * L samples from the state s: steps 1-3.  st(w, n, y) takes output n; a slot reads and writes its own lane's samples
// only and reads sample n before it writes output n, so st may overwrite what ld reads (in place).  Returns the state after the block.
template <int KIND, int L, int W, class X, class LD, class CF, class ST>
MXG_HD S3 swept_block(const X &xch, const S3 &s, LD &&ld, CF &&cf, ST &&st) {
    constexpr int D = swept_dim(KIND);
    SweptLanes<D, W> P;
    swept_lanes<KIND, L, W>(xch, s, ld, cf, P);
    swept_pair_scan<D, W, false>(xch, P);
    double below[D][W], end[D][W];
    for (int i = 0; i < D; i++) xch.up(P.e[i], 1, below[i]);
    for (int w = 0; w < W; w++) {
        const int lane = xch.lane(w);
        const size_t n0 = (size_t)lane * L;
        ScanStep<KIND> step = {};
        S3 t = {below[0][w], D == 2 ? below[D - 1][w] : 0.0, 0.0};
        if (lane == 0) t = s;
        MXG_SCAN_UNROLL
        for (int i = 0; i < L; i++) {
            step.c[0] = cf(w, n0 + i, 0);
            step.c[1] = cf(w, n0 + i, 1);
            st(w, n0 + i, step(t, ld(w, n0 + i)));
        }
        end[0][w] = t.a;
        if constexpr (D == 2) end[D - 1][w] = t.b;
    }
    return S3{xch.from(end[0], kScanLanes - 1), D == 2 ? xch.from(end[D - 1], kScanLanes - 1) : 0.0, 0.0};
}

// Phase B, one voice: the K pairs P_0 .. P_{K-1} (get_p(c)) -> the true states E_0 .. E_{K-1} after those chunks (put_E(c, E)).
template <int D, int W, class X, class GP, class PE>
MXG_HD void swept_chunks(const X &xch, size_t K, GP &&get_p, PE &&put_E) {
    const size_t r = (K + kScanLanes - 1) / kScanLanes;
    SweptLanes<D, W> P;
    for (int w = 0; w < W; w++) {
        const size_t lo = (size_t)xch.lane(w) * r, hi = lo + r < K ? lo + r : K;
        SweptPair p = swept_identity<D>();
        for (size_t c = lo; c < hi; c++) p = c == lo ? get_p(c) : swept_compose<D>(get_p(c), p);
        P.put(w, p);
    }
    swept_pair_scan<D, W, false>(xch, P);
    double below[D][W];
    for (int i = 0; i < D; i++) xch.up(P.e[i], 1, below[i]);
    for (int w = 0; w < W; w++) {
        const size_t lo = (size_t)xch.lane(w) * r, hi = lo + r < K ? lo + r : K;
        S3 s = {below[0][w], D == 2 ? below[D - 1][w] : 0.0, 0.0};
        for (size_t c = lo; c < hi; c++) {
            const SweptPair p = get_p(c);
            s = c == 0 ? p.e : scan_add(swept_apply<D>(p.M, s), p.e);
            put_E(c, s);
        }
    }
}

// The remainder of a voice, R < 1024 samples from the state s: blocks for the set bits of R / 64 from the highest down, then R % 64
// plain steps (ld1(n) / cf1(n, r) / st1(n, y): once per executor).  n counts from the remainder's first sample.
template <int KIND, int W, class X, class LD, class CF, class ST, class LD1, class CF1, class ST1>
MXG_HD S3 swept_tail(const X &xch, S3 s, size_t R, LD &&ld, CF &&cf, ST &&st, LD1 &&ld1, CF1 &&cf1, ST1 &&st1) {
    size_t at = 0;
    auto ldo = [&](int w, size_t n) { return ld(w, at + n); };
    auto cfo = [&](int w, size_t n, int r) { return cf(w, at + n, r); };
    auto sto = [&](int w, size_t n, double y) { st(w, at + n, y); };
    if (R & 512) s = swept_block<KIND, 8, W>(xch, s, ldo, cfo, sto), at += 512;
    if (R & 256) s = swept_block<KIND, 4, W>(xch, s, ldo, cfo, sto), at += 256;
    if (R & 128) s = swept_block<KIND, 2, W>(xch, s, ldo, cfo, sto), at += 128;
    if (R & 64) s = swept_block<KIND, 1, W>(xch, s, ldo, cfo, sto), at += 64;
    ScanStep<KIND> step = {};
    for (; at < R; at++) {
        step.c[0] = cf1(at, 0);
        step.c[1] = cf1(at, 1);
        st1(at, step(s, ld1(at)));
    }
    return s;
}

// ---- the host twin: the three phases over arrays of 64 lane values (plain C++ translation units only) -------------------------
#if !defined(__HIPCC__)
// in / out [N][V] (out == in allowed), coef [N][rows][V], st [NS][V] (NS = 2 rows of [5][V] for lores / hires, 1 for the lag);
// work: (kSweptPairDoubles + kSweptEndDoubles) * (C - 1) doubles for one voice (C = N / 1024), or null if C <= 1
template <int KIND>
inline void scan_long_swept_host_voices(size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out, double *work) {
    constexpr int D = swept_dim(KIND), W = kScanLanes, L = kSweptL;
    const size_t T = kSweptChunk, C = N / T, K = C > 1 ? C - 1 : 0, R = N % T;
    const LongHostXch xch;
    for (size_t v = 0; v < V; v++) {
        S3 s = {st[v], D == 2 ? st[V + v] : 0.0, 0.0};
        const S3 s_in = s;
        double *pairs = work, *ends = work + kSweptPairDoubles * K;
        auto ld_at = [&](size_t n0) { return [=](int, size_t n) { return in[(n0 + n) * V + v]; }; };
        auto cf_at = [&](size_t n0) { return [=](int, size_t n, int r) { return coef[((n0 + n) * rows + r) * V + v]; }; };
        auto st_at = [&](size_t n0) { return [=](int, size_t n, double y) { out[(n0 + n) * V + v] = y; }; };
        for (size_t c = 0; c < K; c++) {  // A
            const SweptPair p = swept_summary<KIND, L, W>(xch, c == 0 ? s_in : S3{0.0, 0.0, 0.0}, ld_at(c * T), cf_at(c * T));
            double *o = pairs + kSweptPairDoubles * c;
            o[0] = p.M.m[0][0], o[1] = p.M.m[0][1], o[2] = p.M.m[1][0], o[3] = p.M.m[1][1], o[4] = p.e.a, o[5] = p.e.b;
        }
        if (K)  // B
            swept_chunks<D, W>(xch, K,
                               [&](size_t c) {
                                   const double *o = pairs + kSweptPairDoubles * c;
                                   SweptPair p = {};
                                   p.M.m[0][0] = o[0], p.M.m[0][1] = o[1], p.M.m[1][0] = o[2], p.M.m[1][1] = o[3], p.e.a = o[4], p.e.b = o[5];
                                   return p;
                               },
                               [&](size_t c, const S3 &q) { ends[kSweptEndDoubles * c] = q.a, ends[kSweptEndDoubles * c + 1] = q.b; });
        for (size_t c = 0; c < C; c++) {  // C
            if (c) s = S3{ends[kSweptEndDoubles * (c - 1)], D == 2 ? ends[kSweptEndDoubles * (c - 1) + 1] : 0.0, 0.0};
            s = swept_block<KIND, L, W>(xch, s, ld_at(c * T), cf_at(c * T), st_at(c * T));
        }
        const size_t n0 = C * T;
        s = swept_tail<KIND, W>(xch, s, R, ld_at(n0), cf_at(n0), st_at(n0), [&](size_t n) { return in[(n0 + n) * V + v]; },
                                [&](size_t n, int r) { return coef[((n0 + n) * rows + r) * V + v]; }, [&](size_t n, double y) { out[(n0 + n) * V + v] = y; });
        st[v] = s.a;
        if (D == 2) st[V + v] = s.b;
    }
}

// Returns 0, or 1 for a kind that has no swept form.
inline int scan_long_swept_host_run(int kind, size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out, double *work) {
    switch (kind) {
        case 3: scan_long_swept_host_voices<3>(V, N, in, coef, rows, st, out, work); return 0;
        case 4: scan_long_swept_host_voices<4>(V, N, in, coef, rows, st, out, work); return 0;
        case 5: scan_long_swept_host_voices<5>(V, N, in, coef, rows, st, out, work); return 0;
    }
    return 1;
}
#endif  // !__HIPCC__

}  // namespace
}  // namespace mxg
