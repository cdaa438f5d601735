// mxg_revfilt.h -- maxiReverbFilters (reference src/libs/maxiReverb.h:42-73, .cpp:3-162) as plain per-sample arithmetic
// (mxg_revfilt_obj.h: every public method of one object, included here), and the custom reverb network built from it:
// P parallel feedback combs summed in order into A serial allpasses, every length a run-time value (revnet.hip, K30).
// Only + - * and compares: the same text compiles for the host (tests/host_revnet.cpp), where rn_voice_ref is the checker
// of the GPU tests.  Compile with contraction off.  The slot arithmetic of a time tile (rv_slot / rv_sub_len / rv_idx_after /
// rv_idx_fix) is mxg_reverb.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mxg_hd.h"
#include "mxg_reverb.h"
#include "mxg_revfilt_obj.h"

namespace mxg {
namespace {

constexpr int RN_MAX = 32;      // = MXG_REVNET_MAX_STAGES: combs, and allpasses, of a network
constexpr int RN_T = 64;        // samples per tile of revnet.hip

// ---- the network: topology and ring layout -------------------------------------------------------------------------
// stage f of a voice: the P combs first, then the A allpasses; ring f at off[f] inside the voice's ring area of S doubles
struct RnLayout {
    int P, A, S;
    uint32_t lpmask;  // bit c: comb c is a low-pass comb (lpcombfb), else plain (combfb)
    int len[2 * RN_MAX], off[2 * RN_MAX];
};
constexpr int RN_OK = 0, RN_BAD_COUNT = 1, RN_BAD_LENGTH = 2, RN_SHORT_LOWPASS = 3;
// 0 <= P, A <= 32, P + A >= 1; every length in [1, 44 100]; a low-pass comb no shorter than the tile, because its
// recurrence is walked over a tile whose ring reads must all be older than the tile
MXG_HD int rn_layout(uint32_t P, uint32_t A, const uint32_t *comb_sizes, const uint32_t *ap_sizes, const uint32_t *comb_lowpass, RnLayout &L) {
    if (P > (uint32_t)RN_MAX || A > (uint32_t)RN_MAX || P + A < 1) return RN_BAD_COUNT;
    if ((P && !comb_sizes) || (A && !ap_sizes)) return RN_BAD_COUNT;
    L.P = (int)P;
    L.A = (int)A;
    L.lpmask = 0;
    int o = 0;
    for (int f = 0; f < 2 * RN_MAX; f++) L.len[f] = L.off[f] = 0;
    for (uint32_t f = 0; f < P + A; f++) {
        const uint32_t D = f < P ? comb_sizes[f] : ap_sizes[f - P];
        if (D < 1 || D > (uint32_t)RF_RING) return RN_BAD_LENGTH;
        if (f < P && comb_lowpass && comb_lowpass[f]) {
            if (D < (uint32_t)RN_T) return RN_SHORT_LOWPASS;
            L.lpmask |= 1u << f;
        }
        L.len[f] = (int)D;
        L.off[f] = o;
        o += (int)D;
    }
    L.S = o;
    return RN_OK;
}
MXG_HD bool rn_is_lp(const RnLayout &L, int c) { return (L.lpmask >> c) & 1u; }

// ---- one voice, one sample at a time, over the bank's state layout ---------------------------------------------------
// rings [V][S] (voice-major), idx int32 [V][P + A], lp [V][P]; comb_fb / comb_cut [V][P], ap_fb [V][A]; in, out [N][V].
struct RnArgs {
    size_t V, N;
    const double *in, *comb_fb, *comb_cut, *ap_fb;
    double *rings;
    int32_t *idx;
    double *lp, *out;
    RnLayout L;
};

MXG_HD void rn_voice_ref(const RnArgs &A, size_t v) {
    const RnLayout &L = A.L;
    const int P = L.P, F = L.P + L.A;
    const size_t V = A.V, N = A.N;
    double *ring = A.rings + v * (size_t)L.S;
    int idx[2 * RN_MAX];
    double y[RN_MAX];
    for (int f = 0; f < F; f++) idx[f] = rv_idx_fix(A.idx[v * F + f], L.len[f]);
    for (int c = 0; c < P; c++) y[c] = rn_is_lp(L, c) ? A.lp[v * P + c] : 0.0;
    for (size_t n = 0; n < N; n++) {
        const double x = A.in[n * V + v];
        double acc = 0.0;
        for (int c = 0; c < P; c++) {
            double *slot = ring + L.off[c] + idx[c];
            const double fb = A.comb_fb[v * P + c];
            double o;
            if (rn_is_lp(L, c)) {
                y[c] = rf_lopass(y[c], rf_lp_coef(A.comb_cut[v * P + c]), *slot);
                o = rf_combfb(x, fb, y[c]);
            } else {
                o = rf_combfb(x, fb, *slot);
            }
            *slot = o;
            idx[c] = idx[c] != L.len[c] - 1 ? idx[c] + 1 : 0;
            acc += o;
        }
        double t = P ? acc : x;
        for (int f = P; f < F; f++) {
            double *slot = ring + L.off[f] + idx[f];
            *slot = rf_allpass(*slot, A.ap_fb[v * L.A + (f - P)], t);
            idx[f] = idx[f] != L.len[f] - 1 ? idx[f] + 1 : 0;
        }
        A.out[n * V + v] = t;
    }
    for (int f = 0; f < F; f++) A.idx[v * F + f] = idx[f];
    for (int c = 0; c < P; c++)
        if (rn_is_lp(L, c)) A.lp[v * P + c] = y[c];
}

}  // namespace
}  // namespace mxg
