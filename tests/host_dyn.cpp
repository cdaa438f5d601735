// tests/host_dyn.cpp -- host build of mxg_dyn.h (tests/test_dyn_host.py; the checker of tests/test_gpu_dyn.py).
// dyn_host_render / rms_host_render take the arguments of mxg_dynamics_render / mxg_rms_render (include/maxigpu.h)
// without the stream, on host arrays in the same layouts, and run dyn_voice_block / rms_voice_block -- the function a
// lane of dyn.hip's kernels runs -- voice after voice.  log10 / pow / sqrt are the host libm's here, as in the reference.
#include <stdint.h>

#include <thread>
#include <vector>

#include "mxg_dyn.h"

using namespace mxg;

// voices are independent: large banks are split over a few threads (same arithmetic, same bits)
template <class F>
static void for_voices(size_t V, F f) {
    const size_t T = V >= 4096 ? 8 : 1;
    if (T == 1) {
        for (size_t v = 0; v < V; v++) f(v);
        return;
    }
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; t++)
        th.emplace_back([=] {
            for (size_t v = V * t / T; v < V * (t + 1) / T; v++) f(v);
        });
    for (auto &x : th) x.join();
}

extern "C" {

int dyn_host_render(size_t V, size_t N, const double *sig, const double *control, const double *th, const double *rh,
                    const double *kh, const double *tl, const double *rl, const double *kl, int ps, const uint32_t *window,
                    const uint32_t *look, const int32_t *analyser, const double *tab_h, const double *tab_l, int nstages,
                    double *rring, size_t cap_r, double *lring, size_t cap_l, int32_t *rpos, int32_t *lpos, double *running,
                    double *dst_h, int64_t *ist_h, double *dst_l, int64_t *ist_l, uint32_t *ovf, double *out,
                    double *level_db) {
    const DynArgs A = {V, N, sig, control, {th, rh, kh, tl, rl, kl}, ps, window, look, analyser, tab_h, tab_l, nstages,
                       rring, (int)cap_r, lring, (int)cap_l, rpos, lpos, running, dst_h, ist_h, dst_l, ist_l, ovf, out,
                       level_db};
    for_voices(V, [&A, tab_h, tab_l](size_t v) { dyn_voice_block(A, v, tab_h, tab_l); });
    return 0;
}

int rms_host_render(size_t V, size_t N, const double *in, const uint32_t *window, double *ring, size_t cap, int32_t *pos,
                    double *running, uint32_t *ovf, double *out) {
    const RmsArgs A = {V, N, in, window, ring, (int)cap, pos, running, ovf, out};
    for_voices(V, [&A](size_t v) { rms_voice_block(A, v); });
    return 0;
}

int dyn_host_set_time(double *tab, size_t S, size_t index, double ms, double sr) {
    return dyn_envgen_set_time(tab, S, index, ms, sr);
}

// the ring index logic, one call per operation
int dyn_host_ring_advance(int idx, int size) { return dyn_ring_advance(idx, size); }
int dyn_host_ring_tail(int idx, int size, int n) { return dyn_ring_tail_slot(idx, size, n); }
int dyn_host_ring_head(int idx, int size) { return dyn_ring_head_slot(idx, size); }

}  // extern "C"
