// tests/host_revnet.cpp -- host build of mxg_revfilt.h (tests/revnet_host.py).
//   rn_host_render: a bank rendered one voice and one sample at a time (rn_voice_ref) over the layout of mxg_revnet_render,
//                   voices spread over threads.  The checker of the golden file and of the GPU tests.
//   rn_host_tiled:  the same bank rendered the way revnet.hip does it: tiles of 64 samples, one stage after the other over
//                   the whole tile; on a ring of D >= 64 slots every read of the tile before any write, slots from rv_slot;
//                   a low-pass comb's recurrence walked over the tile's reads; a shorter ring in sub-tiles of rv_sub_len
//                   samples, inside a sub-tile every read before any write; the index advanced once per tile by rv_idx_after.
//                   Returns the number of slot collisions inside a parallel pass (0 where the tile rule holds).
//   rn_host_layout: rn_layout's answer.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "mxg_revfilt.h"

using namespace mxg;

static RnArgs make_args(const RnLayout &L, size_t V, size_t N, const double *in, const double *comb_fb, const double *comb_cut,
                        const double *ap_fb, double *rings, int32_t *idx, double *lp, double *out) {
    return RnArgs{V, N, in, comb_fb, comb_cut, ap_fb, rings, idx, lp, out, L};
}

extern "C" int rn_host_layout(uint32_t P, uint32_t A, const uint32_t *comb_sizes, const uint32_t *ap_sizes, const uint32_t *lowpass,
                              int32_t *offs, int32_t *S) {
    RnLayout L;
    if (int s = rn_layout(P, A, comb_sizes, ap_sizes, lowpass, L)) return s;
    for (int f = 0; f < L.P + L.A; f++) offs[f] = L.off[f];
    *S = L.S;
    return 0;
}

extern "C" int rn_host_render(uint32_t P, uint32_t A, const uint32_t *comb_sizes, const uint32_t *ap_sizes, const uint32_t *lowpass, size_t V,
                              size_t N, const double *in, const double *comb_fb, const double *comb_cut, const double *ap_fb, double *rings,
                              int32_t *idx, double *lp, double *out, int nthreads) {
    RnLayout L;
    if (int s = rn_layout(P, A, comb_sizes, ap_sizes, lowpass, L)) return s;
    const RnArgs Ar = make_args(L, V, N, in, comb_fb, comb_cut, ap_fb, rings, idx, lp, out);
    if (nthreads < 1) nthreads = 1;
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++)
        th.emplace_back([&Ar, t, nthreads] {
            for (size_t v = t; v < Ar.V; v += nthreads) rn_voice_ref(Ar, v);
        });
    for (auto &x : th) x.join();
    return 0;
}

namespace {
// one stage over one tile: v[i] is sample i's value in (the input for a comb, the chain for an allpass), o[i] its output
int stage_tile(bool comb, bool lowpass, double *ring, int D, int i0, double g, double coef, double &y, const double *v, double *o, int nt) {
    int bad = 0;
    const int T = RN_T;
    std::vector<int> sl(T);
    std::vector<double> d(T);
    if (D >= T) {
        for (int i = 0; i < nt; i++) {
            sl[i] = rv_slot(i0, i, D);
            if (sl[i] != (i0 + i) % D) bad++;
            d[i] = ring[sl[i]];
        }
        if (lowpass)
            for (int i = 0; i < nt; i++) d[i] = y = rf_lopass(y, coef, d[i]);
        for (int i = nt - 1; i >= 0; i--) {  // any order: the slots are distinct
            if (comb) {
                o[i] = rf_combfb(v[i], g, d[i]);
                ring[sl[i]] = o[i];
            } else {
                o[i] = v[i];
                ring[sl[i]] = rf_allpass(d[i], g, o[i]);
            }
            for (int j = 0; j < i; j++)
                if (sl[j] == sl[i]) bad++;
        }
        return bad;
    }
    if (lowpass) return 1 << 20;  // the layout rule forbids it
    const int L = rv_sub_len(D, 1, T);
    for (int s0 = 0; s0 < nt; s0 += L) {
        const int s1 = s0 + L < nt ? s0 + L : nt;
        for (int i = s0; i < s1; i++) {
            sl[i] = (i0 + i) % D;
            d[i] = ring[sl[i]];
        }
        for (int i = s1 - 1; i >= s0; i--) {
            if (comb) {
                o[i] = rf_combfb(v[i], g, d[i]);
                ring[sl[i]] = o[i];
            } else {
                o[i] = v[i];
                ring[sl[i]] = rf_allpass(d[i], g, o[i]);
            }
            for (int j = s0; j < i; j++)
                if (sl[j] == sl[i]) bad++;
        }
    }
    return bad;
}

int voice_tiled(const RnArgs &A, size_t v) {
    const RnLayout &L = A.L;
    const int P = L.P, F = L.P + L.A, T = RN_T;
    const size_t V = A.V, N = A.N;
    double *ring = A.rings + v * (size_t)L.S;
    int bad = 0;
    std::vector<int> idx(F);
    std::vector<double> y(P ? P : 1, 0.0);
    for (int f = 0; f < F; f++) idx[f] = rv_idx_fix(A.idx[v * F + f], L.len[f]);
    for (int c = 0; c < P; c++)
        if (rn_is_lp(L, c)) y[c] = A.lp[v * P + c];
    double x[RN_T], acc[RN_T], o[RN_T];
    for (size_t n0 = 0; n0 < N; n0 += T) {
        const int nt = (int)(N - n0 < (size_t)T ? N - n0 : (size_t)T);
        for (int i = 0; i < nt; i++) {
            x[i] = A.in[(n0 + i) * V + v];
            acc[i] = 0.0;
        }
        for (int c = 0; c < P; c++) {
            const bool lp = rn_is_lp(L, c);
            bad += stage_tile(true, lp, ring + L.off[c], L.len[c], idx[c], A.comb_fb[v * P + c], lp ? rf_lp_coef(A.comb_cut[v * P + c]) : 0.0,
                              y[c], x, o, nt);
            for (int i = 0; i < nt; i++) acc[i] += o[i];
        }
        double *t = P ? acc : x;
        for (int f = P; f < F; f++) {
            double dummy = 0.0;
            bad += stage_tile(false, false, ring + L.off[f], L.len[f], idx[f], A.ap_fb[v * L.A + (f - P)], 0.0, dummy, t, o, nt);
            for (int i = 0; i < nt; i++) t[i] = o[i];
        }
        for (int i = 0; i < nt; i++) A.out[(n0 + i) * V + v] = t[i];
        for (int f = 0; f < F; f++) idx[f] = rv_idx_after(idx[f], nt, L.len[f]);
    }
    for (int f = 0; f < F; f++) A.idx[v * F + f] = idx[f];
    for (int c = 0; c < P; c++)
        if (rn_is_lp(L, c)) A.lp[v * P + c] = y[c];
    return bad;
}
}  // namespace

extern "C" int rn_host_tiled(uint32_t P, uint32_t A, const uint32_t *comb_sizes, const uint32_t *ap_sizes, const uint32_t *lowpass, size_t V,
                             size_t N, const double *in, const double *comb_fb, const double *comb_cut, const double *ap_fb, double *rings,
                             int32_t *idx, double *lp, double *out) {
    RnLayout L;
    if (int s = rn_layout(P, A, comb_sizes, ap_sizes, lowpass, L)) return -s;
    const RnArgs Ar = make_args(L, V, N, in, comb_fb, comb_cut, ap_fb, rings, idx, lp, out);
    int bad = 0;
    for (size_t v = 0; v < V; v++) bad += voice_tiled(Ar, v);
    return bad;
}
