// tests/host_fx.cpp -- host build of mxg_fx.h (tests/test_fx_host.py).  For random size sequences it checks the tile
// machinery of fx.hip against the plain step-by-step recurrence of maxiDelayline::dl (C:420-429):
//   - the slots fx_ring_slot produces are the recurrence's;
//   - every slot of a tile lies in the classifier's two runs [a0, a0+k) and [0, m), m <= T;
//   - the tile is classed conflict-free exactly when its slots are distinct;
//   - the staging map is injective on the touched set and stays in [0, 2T); the staged slots cover it once;
//   - a ring updated tile by tile the kernel's way (parallel when conflict-free, a staged walk otherwise) equals
//     the ring updated one sample at a time.
// Returns the number of failed checks.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "mxg_fx.h"

using namespace mxg;

extern "C" int fx_tile_fuzz(int T, int cap, int nsamp, const double *sizes_d, int ph0, const double *in, double fb,
                            int *n_conflicted) {
    int bad = 0;
    std::vector<double> ring_a(cap, 0.0), ring_b(cap, 0.0);
    for (int i = 0; i < cap; i++) ring_a[i] = ring_b[i] = 0.001 * i;
    int ph_ref = ph0, ph = ph0;
    uint32_t ovf = 0, ovf_ref = 0;
    std::vector<int> slots(T);
    std::vector<double> stg(2 * T), o_a(T), o_b(T);
    std::vector<int> home(2 * T);
    *n_conflicted = 0;
    for (int n0 = 0; n0 < nsamp; n0 += T) {
        const int nt = nsamp - n0 < T ? nsamp - n0 : T;
        FxTile t;
        fx_tile_begin(t);
        for (int i = 0; i < nt; i++) {
            const int s = fx_ring_slot(ph, fx_ring_size(fx_cvt_i32(sizes_d[n0 + i]), cap, ovf));
            // the plain recurrence, written out
            const int si = fx_cvt_i32(sizes_d[n0 + i]);
            int sz = si;
            if (sz > cap) {
                sz = cap;
                ovf_ref++;
            }
            if (ph_ref < 0 || ph_ref >= sz) ph_ref = 0;
            const int sref = ph_ref++;
            if (s != sref) bad++;
            slots[i] = s;
            fx_tile_add(t, i, s);
        }
        // touched set, conflict class
        bool distinct = true;
        for (int i = 0; i < nt; i++) {
            const int s = slots[i];
            if (!((s >= t.a0 && s < t.a0 + t.k) || s < t.m)) bad++;
            for (int j = 0; j < i; j++)
                if (slots[j] == s) distinct = false;
        }
        if (t.m > T || t.k > T) bad++;
        if (fx_tile_conflict(t) == distinct) bad++;
        if (!distinct) (*n_conflicted)++;
        // staging: homes of the staged slots are distinct, in range, and every touched slot has one
        for (int j = 0; j < 2 * T; j++) home[j] = -1;
        for (int j = 0; j < T; j++) {
            const int sa = fx_stage_slot_a(t, j), sb = fx_stage_slot_b(t, j);
            if (sa >= 0) {
                const int h = fx_stage_index(t, sa, T);
                if (h != j || home[h] != -1) bad++;
                else home[h] = sa;
            }
            if (sb >= 0) {
                const int h = fx_stage_index(t, sb, T);
                if (h != T + j || home[h] != -1) bad++;
                else home[h] = sb;
            }
        }
        for (int i = 0; i < nt; i++) {
            const int h = fx_stage_index(t, slots[i], T);
            if (h < 0 || h >= 2 * T || home[h] != slots[i]) bad++;
        }
        // ring A: one sample at a time
        for (int i = 0; i < nt; i++) {
            o_a[i] = ring_a[slots[i]];
            ring_a[slots[i]] = fx_ring_update(ring_a[slots[i]], in[n0 + i], fb);
        }
        // ring B: the kernel's way
        if (!fx_tile_conflict(t)) {
            for (int i = nt - 1; i >= 0; i--) {  // any order: the updates are independent
                const double c = ring_b[slots[i]];
                o_b[i] = c;
                ring_b[slots[i]] = fx_ring_update(c, in[n0 + i], fb);
            }
        } else {
            for (int j = 0; j < 2 * T; j++)
                if (home[j] >= 0) stg[j] = ring_b[home[j]];
            for (int i = 0; i < nt; i++) {
                const int h = fx_stage_index(t, slots[i], T);
                o_b[i] = stg[h];
                stg[h] = fx_ring_update(stg[h], in[n0 + i], fb);
            }
            for (int j = 0; j < 2 * T; j++)
                if (home[j] >= 0) ring_b[home[j]] = stg[j];
        }
        for (int i = 0; i < nt; i++)
            if (memcmp(&o_a[i], &o_b[i], 8)) bad++;
    }
    if (memcmp(ring_a.data(), ring_b.data(), 8 * (size_t)cap)) bad++;
    if (ph != ph_ref || ovf != ovf_ref) bad++;
    return bad;
}

// the per-sample arithmetic of mxg_fx.h over one voice, for the comparison with tests/fx_port.py
extern "C" void fx_flanger_host(int N, const double *in, uint32_t delay, double fb, double speed, double depth, double sr,
                                int cap, double *out) {
    std::vector<double> mem(cap, 0.0);
    int ph = 0;
    uint32_t ovf = 0;
    double lph = 0.0;
    const double inc = fx_tri_inc(sr, speed);
    for (int n = 0; n < N; n++) {
        const double lfo = fx_triangle(lph, inc);
        const int s = fx_ring_slot(ph, fx_ring_size(fx_flanger_size(delay, lfo, depth), cap, ovf));
        const double o = mem[s];
        mem[s] = fx_ring_update(o, in[n], fb);
        out[n] = fx_flanger_out(o, in[n]);
    }
}

extern "C" void fx_chorus_host(int N, const double *in, uint32_t delay, double fb, double c, double r, double depth,
                               const int32_t *rnd, int cap, double *out) {
    std::vector<double> m1(cap, 0.0), m2(cap, 0.0);
    int p1 = 0, p2 = 0;
    uint32_t ovf = 0;
    double x = 0.0, y = 0.0;
    for (int n = 0; n < N; n++) {
        const double lfo = fx_lores(x, y, fx_noise(rnd[n]), c, r) * 2.0;
        const int s1 = fx_ring_slot(p1, fx_ring_size(fx_flanger_size(delay, lfo, depth), cap, ovf));
        const int s2 = fx_ring_slot(p2, fx_ring_size(fx_chorus_size2(delay, lfo, depth), cap, ovf));
        const double o1 = m1[s1], o2 = m2[s2];
        m1[s1] = fx_ring_update(o1, in[n], fb);
        m2[s2] = fx_ring_update(o2, in[n], fb * 0.99);
        out[n] = fx_chorus_out(o1, o2, in[n]);
    }
}
