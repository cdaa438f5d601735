// tests/host_dattaro.cpp -- host build of mxg_dattaro.h (tests/dattaro_host.py).
//   dt_host_render: a bank rendered one voice and one sample at a time (dt_voice_ref) over the layout of mxg_dattaro_render,
//                   voices spread over threads.  The checker of the golden file and of the GPU tests.
//   dt_host_layout: lengths, offsets, tap positions and tap rings of a sample rate; returns the ring doubles per voice, or -1
//                   where the rate is not accepted.
//   dt_tile_fuzz:   one voice rendered tile by tile the way dattaro.hip does it (every read of a tile's tank slots and taps
//                   before any of its writes, taps at distance 0 from the sample's own write, the input rings in sub-tiles of
//                   dt_in_sub_len samples, sigl / sigr from the previous sample's reads of D1 / D3, indices advanced per tile)
//                   against dt_voice_ref.  Returns the number of differing values.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "mxg_dattaro.h"

using namespace mxg;

extern "C" int dt_host_layout(uint32_t sample_rate, int32_t *lens, int32_t *offs, int32_t *taps, int32_t *tap_rings) {
    const DtLayout L = dt_layout(sample_rate);
    for (int r = 0; r < DT_RINGS; r++) {
        if (lens) lens[r] = L.len[r];
        if (offs) offs[r] = L.off[r];
    }
    for (int j = 0; j < DT_TAPS; j++) {
        if (taps) taps[j] = L.tap[j];
        if (tap_rings) tap_rings[j] = dt_tap_ring(j);
    }
    return dt_accepts(L, 64) ? L.S : -1;
}

extern "C" int dt_host_render(uint32_t sample_rate, size_t V, size_t N, const double *in, double *rings, int32_t *idx, double *state,
                              double *out, int nthreads) {
    const DtLayout L = dt_layout(sample_rate);
    if (!dt_accepts(L, 64)) return -1;
    const DtArgs A = {V, N, in, rings, idx, state, out, L};
    if (nthreads < 1) nthreads = 1;
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++)
        th.emplace_back([&A, t, nthreads] {
            for (size_t v = t; v < A.V; v += nthreads) dt_voice_ref(A, v);
        });
    for (auto &x : th) x.join();
    return 0;
}

static int diff(const void *a, const void *b, size_t n) {  // differing 8-byte words
    int bad = 0;
    for (size_t i = 0; i < n; i++) bad += memcmp((const char *)a + 8 * i, (const char *)b + 8 * i, 8) != 0;
    return bad;
}

// one voice; rings / idx / state hold the start state and are left untouched
extern "C" int dt_tile_fuzz(uint32_t sample_rate, int T, size_t N, const double *in, const double *rings, const int32_t *idx,
                            const double *state) {
    const DtLayout L = dt_layout(sample_rate);
    if (!dt_accepts(L, T)) return -1;
    // A: one sample at a time
    std::vector<double> ra(rings, rings + L.S), sa(state, state + DT_STATE), oa(2 * N);
    std::vector<int32_t> ia(idx, idx + DT_RINGS);
    const DtArgs A = {1, N, in, ra.data(), ia.data(), sa.data(), oa.data(), L};
    dt_voice_ref(A, 0);
    // B: the kernel's way
    std::vector<double> rb(rings, rings + L.S), ob(2 * N);
    double *ring = rb.data();
    int ix[DT_RINGS];
    for (int r = 0; r < DT_RINGS; r++) ix[r] = dt_idx_fix(idx[r], L.len[r]);
    double y[3] = {state[DT_LP0], state[DT_LP1], state[DT_LP2]}, sig[2] = {state[DT_SIGL], state[DT_SIGR]};
    std::vector<double> lp0(T), lp1(T), lp2(T), d(T), old((size_t)T * DT_RINGS), tp((size_t)T * DT_TAPS), wr(DT_RINGS);
    for (size_t n0 = 0; n0 < N; n0 += T) {
        const int nt = N - n0 < (size_t)T ? (int)(N - n0) : T;
        for (int k = 0; k < nt; k++) {  // the low-passes, in order
            lp0[k] = y[0] = dt_lopass(y[0], 0.8, in[n0 + k]);
            lp1[k] = y[1] = dt_lopass(y[1], 0.4, ring[L.off[DT_D0] + dt_slot(ix[DT_D0], k, L.len[DT_D0])]);
            lp2[k] = y[2] = dt_lopass(y[2], 0.4, ring[L.off[DT_D2] + dt_slot(ix[DT_D2], k, L.len[DT_D2])]);
        }
        for (int k = 0; k < nt; k++) {  // every read of the tank
            for (int r = 2; r < DT_RINGS; r++) old[k * DT_RINGS + r] = ring[L.off[r] + dt_slot(ix[r], k, L.len[r])];
            for (int j = 0; j < DT_TAPS; j++) {
                const int r = dt_tap_ring(j);
                tp[k * DT_TAPS + j] = ring[L.off[r] + dt_tap_slot(ix[r], k, L.tap[j], L.len[r])];
            }
        }
        const int D0 = L.len[DT_AP0], D1 = L.len[DT_AP1], Ls = dt_in_sub_len(D0, D1, T);
        for (int s0 = 0; s0 < nt; s0 += Ls)
            for (int k = (s0 + Ls < nt ? s0 + Ls : nt) - 1; k >= s0; k--) {  // any order inside a sub-tile
                double t = lp0[k];
                double *a0 = ring + L.off[DT_AP0] + (ix[DT_AP0] + 2 * k) % D0, *a1 = ring + L.off[DT_AP0] + (ix[DT_AP0] + 2 * k + 1) % D0;
                double *b0 = ring + L.off[DT_AP1] + (ix[DT_AP1] + 2 * k) % D1, *b1 = ring + L.off[DT_AP1] + (ix[DT_AP1] + 2 * k + 1) % D1;
                if (Ls == T && (a0 != ring + L.off[DT_AP0] + dt_slot(ix[DT_AP0], 2 * k, D0) || b1 != ring + L.off[DT_AP1] + dt_slot(ix[DT_AP1], 2 * k + 1, D1)))
                    return -2;
                *a0 = dt_allpass(*a0, t, 0.75);
                *b0 = dt_allpass(*b0, t, 0.75);
                *a1 = dt_allpass(*a1, t, 0.625);
                *b1 = dt_allpass(*b1, t, 0.625);
                d[k] = t;
            }
        for (int k = nt - 1; k >= 0; k--) {  // the tank, any order
            const double *o = &old[k * DT_RINGS];
            const double pl = k ? old[(k - 1) * DT_RINGS + DT_D1] : sig[0], pr = k ? old[(k - 1) * DT_RINGS + DT_D3] : sig[1];
            double tl = dt_cross(d[k], pr), tr = dt_cross(d[k], pl);
            wr[DT_AP4] = dt_allpass(o[DT_AP4], tl, 0.7);
            wr[DT_D0] = tl;
            tl = lp1[k];
            wr[DT_AP5] = dt_allpass(o[DT_AP5], tl, 0.5);
            wr[DT_D1] = tl;
            wr[DT_AP6] = dt_allpass(o[DT_AP6], tr, 0.7);
            wr[DT_D2] = tr;
            tr = lp2[k];
            wr[DT_AP7] = dt_allpass(o[DT_AP7], tr, 0.5);
            wr[DT_D3] = tr;
            for (int r = 2; r < DT_RINGS; r++) ring[L.off[r] + dt_slot(ix[r], k, L.len[r])] = wr[r];
            double *t = &tp[k * DT_TAPS];
            for (int j = 0; j < DT_TAPS; j++)
                if (dt_tap_dist(L.len[dt_tap_ring(j)], L.tap[j]) == 0) t[j] = wr[dt_tap_ring(j)];
            ob[n0 + k] = dt_mix(t[0], t[1], t[2], t[3], t[4], t[5], t[6]);
            ob[N + n0 + k] = dt_mix(t[7], t[8], t[9], t[10], t[11], t[12], t[13]);
        }
        sig[0] = old[(nt - 1) * DT_RINGS + DT_D1];
        sig[1] = old[(nt - 1) * DT_RINGS + DT_D3];
        for (int r = 0; r < DT_RINGS; r++) ix[r] = dt_idx_after(ix[r], dt_steps(r) * nt, L.len[r]);
    }
    int bad = diff(oa.data(), ob.data(), 2 * N) + diff(ra.data(), rb.data(), (size_t)L.S);
    for (int r = 0; r < DT_RINGS; r++) bad += ix[r] != ia[r];
    const double sb[DT_STATE] = {y[0], y[1], y[2], sig[0], sig[1]};
    return bad + diff(sa.data(), sb, DT_STATE);
}
