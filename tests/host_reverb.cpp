// tests/host_reverb.cpp -- host build of mxg_reverb.h (tests/reverb_host.py).
//   rv_host_render: a bank rendered one voice and one sample at a time (rv_voice_ref) over the layout of mxg_reverb_render,
//                   voices spread over threads.  The checker of the golden file and of the GPU tests.
//   rv_tile_fuzz:   one allpass ring of D slots stepped `steps` times per sample, updated tile by tile the way reverb.hip
//                   does it (sub-tiles of rv_sub_len samples, inside a sub-tile every read before any write, slots from
//                   rv_slot where the tile fits the ring, the index advanced by rv_idx_after) against the step-by-step
//                   recurrence.  Returns the number of failed checks.
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "mxg_reverb.h"

using namespace mxg;

template <int KIND>
static void run_bank(const RvArgs &A, int nthreads) {
    if (nthreads < 1) nthreads = 1;
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++)
        th.emplace_back([&A, t, nthreads] {
            for (size_t v = t; v < A.V; v += nthreads) rv_voice_ref<KIND>(A, v);
        });
    for (auto &x : th) x.join();
}

extern "C" int rv_host_render(int kind, int mode, size_t V, size_t N, const double *in, const double *room, const double *absorb,
                              int ps, double *rings, int32_t *idx, double *lp, double *wc, double *out, int nthreads) {
    const RvArgs A = {mode, V, N, in, room, absorb, ps, rings, idx, lp, wc, out};
    if (kind == RV_SAT) run_bank<RV_SAT>(A, nthreads);
    else if (kind == RV_FREEVERB) run_bank<RV_FREEVERB>(A, nthreads);
    else if (kind == RV_STEREO) run_bank<RV_STEREO>(A, nthreads);
    else return -1;
    return 0;
}

extern "C" int rv_layout(int kind, int32_t *lens, int32_t *offs) {
    for (int f = 0; f < rv_nfilt(kind); f++) {
        lens[f] = rv_len(kind, f);
        offs[f] = rv_off(kind, f);
    }
    return rv_ring_doubles(kind);
}

// in [steps][N]: the stage's input per pass (pass 0 then pass 1 inside a sample); idx0 may lie outside the ring
extern "C" int rv_tile_fuzz(int T, int D, int steps, int idx0, int N, const double *in) {
    int bad = 0;
    std::vector<double> ra(D), rb(D), oa((size_t)steps * N), ob((size_t)steps * N);
    for (int i = 0; i < D; i++) ra[i] = rb[i] = 0.001 * i - 0.01;
    // A: one step at a time
    int ia = rv_idx_fix(idx0, D);
    for (int n = 0; n < N; n++)
        for (int p = 0; p < steps; p++) {
            double t = in[(size_t)p * N + n];
            ra[ia] = rv_allpass(ra[ia], t);
            ia = ia != D - 1 ? ia + 1 : 0;
            oa[(size_t)p * N + n] = t;
        }
    // B: the kernel's way
    int ib = rv_idx_fix(idx0, D);
    const int L = rv_sub_len(D, steps, T);
    if (L < 1) return -1;
    std::vector<double> d((size_t)steps * T);
    std::vector<int> sl((size_t)steps * T);
    for (int n0 = 0; n0 < N; n0 += T) {
        const int nt = N - n0 < T ? N - n0 : T;
        for (int s0 = 0; s0 < nt; s0 += L) {
            const int s1 = s0 + L < nt ? s0 + L : nt;
            for (int i = s0; i < s1; i++)
                for (int p = 0; p < steps; p++) {
                    int s = (ib + steps * i + p) % D;
                    if (steps * T <= D && s != rv_slot(ib, steps * i + p, D)) bad++;
                    sl[i * steps + p] = s;
                    d[i * steps + p] = rb[s];
                }
            for (int i = s1 - 1; i >= s0; i--)  // any order: the slots of a sub-tile are distinct
                for (int p = 0; p < steps; p++) {
                    double t = in[(size_t)p * N + n0 + i];
                    rb[sl[i * steps + p]] = rv_allpass(d[i * steps + p], t);
                    ob[(size_t)p * N + n0 + i] = t;
                }
            for (int a = s0 * steps; a < s1 * steps; a++)
                for (int b = s0 * steps; b < a; b++)
                    if (sl[a] == sl[b]) bad++;
        }
        ib = rv_idx_after(ib, steps * nt, D);
    }
    if (ia != ib) bad++;
    if (memcmp(ra.data(), rb.data(), 8 * (size_t)D)) bad++;
    if (memcmp(oa.data(), ob.data(), 8 * oa.size())) bad++;
    return bad;
}
