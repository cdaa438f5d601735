// tests/host_looper.cpp -- host build of mxg_looper.h (tests/test_looper_host.py; pinned to tests/golden/looper.npz).
// lp_h_render / lp_h_normalise take the arguments of mxg_looprec_render / mxg_sample_pool_normalise (include/maxigpu.h) without
// cap and the stream, on host arrays in the pool's layout, and run the functions the kernels of looper.hip run.  lp_h_play_step
// and lp_h_smp_step are one call of the players as mxg_looper.h restates them and as mxg_smp.h has them (smp_gen<0> / <2>), side
// by side.  With -DLOOPER_HOST_MAIN the file is a stand-alone program that plays small pools over every special value, bounds
// inside and outside [0, 1] and blocks cut at every position (the sanitizer run).
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <utility>
#include <vector>

#include "mxg_smp.h"
#include "mxg_looper.h"

using namespace mxg;

extern "C" {

int lp_h_render(size_t R, size_t N, double *pool, size_t stride, const uint64_t *len, const double *in, const double *enable, int eps,
                const double *mix, const double *start, const double *end, double *recpos, double *lagval, int play_mode,
                const double *pstart, const double *pend, double *position, double *out, uint32_t *dropped) {
    lp_host_render(R, N, pool, stride, len, in, enable, eps, mix, start, end, recpos, lagval, play_mode, pstart, pend, position, out, dropped);
    return 0;
}

// The same call as K25 cuts it (looper.hip): pieces of `piece` samples, tiles of `tile` slots with their entries side by side,
// lp_plan_slot per slot, then every first visit's element loaded and walked (lp_walk_element) and every play-head read of an
// element the piece does not record on -- all loads of a piece before its first store, as the kernel's barrier has it.
int lp_h_render_pieces(int piece, int tile, size_t R, size_t N, double *pool, size_t stride, const uint64_t *len, const double *in,
                       const double *enable, int eps, const double *mix, const double *start, const double *end, double *recpos,
                       double *lagval, int play_mode, const double *pstart, const double *pend, double *position, double *out,
                       uint32_t *dropped) {
    const size_t E = (size_t)piece * tile;
    std::vector<double> sVal(E), sEn(E), sLag(E), pv(E);
    std::vector<int> sIdx(E), sLink(E), sPlay(E);
    const bool playing = play_mode != MXG_LOOPER_PLAY_NONE;
    for (size_t n0 = 0; n0 < N; n0 += piece) {
        const int Np = (int)(N - n0 < (size_t)piece ? N - n0 : (size_t)piece);
        for (size_t r0 = 0; r0 < R; r0 += tile) {
            const int nT = (int)(R - r0 < (size_t)tile ? R - r0 : (size_t)tile);
            for (int n = 0; n < Np; n++)
                for (int s = 0; s < nT; s++) {
                    sVal[n * tile + s] = in[(n0 + n) * R + r0 + s];
                    if (eps) sEn[n * tile + s] = enable[(n0 + n) * R + r0 + s];
                }
            for (int s = 0; s < nT; s++) {
                const size_t r = r0 + s;
                LpRec rec = {recpos[r], lagval[r]};
                double pos = playing ? position[r] : 0.0;
                uint32_t drops = 0;
                lp_plan_slot(Np, tile, (size_t)len[r], eps ? sEn.data() + s : nullptr, eps ? false : enable[r] != 0.0, start[r], end[r], play_mode,
                             playing && pstart ? pstart[r] : 0.0, playing && pend ? pend[r] : 0.0, rec, pos, drops, sLag.data() + s, sIdx.data() + s,
                             sLink.data() + s, sPlay.data() + s);
                recpos[r] = rec.recpos;
                lagval[r] = rec.lag;
                if (playing) position[r] = pos;
                if (dropped) dropped[r] += drops;
            }
            std::vector<std::pair<double *, double>> stores;
            for (int n = 0; n < Np; n++)
                for (int s = 0; s < nT; s++) {
                    const int e = n * tile + s;
                    double *slot = pool + (r0 + s) * stride;
                    if (sLink[e] & kLpLinkHead) {
                        double *p = slot + sIdx[e];
                        double c = *p;
                        if (lp_walk_element(n, tile, mix[r0 + s], c, sVal.data() + s, sLag.data() + s, sLink.data() + s)) stores.push_back({p, c});
                    }
                    if (playing && sPlay[e] < 0) pv[e] = slot[(long long)(-sPlay[e]) - 6];
                }
            for (auto &st : stores) *st.first = st.second;
            if (playing)
                for (int n = 0; n < Np; n++)
                    for (int s = 0; s < nT; s++) {
                        const int e = n * tile + s;
                        out[(n0 + n) * R + r0 + s] = sPlay[e] >= 0 ? sVal[sPlay[e] * tile + s] : pv[e];
                    }
        }
    }
    return 0;
}

int lp_h_normalise(size_t R, double *pool, size_t stride, const uint64_t *len, const double *maxLevel) {
    lp_host_normalise(R, pool, stride, len, maxLevel);
    return 0;
}

long long lp_h_play_step(int mode, double *pos, double start, double end, size_t len) { return lp_play_step(mode, *pos, start, end, len); }

long long lp_h_smp_step(int mode, double *pos, double start, double end, size_t len) {
    Smp s = {nullptr, len, *pos, 1.0, 0.0, false, 0.0, 0.0};
    long long idx;
    if (mode == 0) {
        SmpReq<0> q;
        smp_gen<0>(s, 0.0, 0.0, start, end, 44100.0, q);
        idx = q.idx[0];
    } else {
        SmpReq<2> q;
        smp_gen<2>(s, 0.0, 0.0, start, end, 44100.0, q);
        idx = q.idx[0];
    }
    *pos = s.pos;
    return idx;
}

int lp_h_guards(int *lo, int *hi) {
    *lo = kSmpGuardLo;
    *hi = kSmpGuardHi;
    return 0;
}

}  // extern "C"

#ifdef LOOPER_HOST_MAIN
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double special[] = {-inf, -1.5, -0.0, 0.0, 0.25, 0.5, 0.999, 1.0, 1.5, inf, nan, 1e-310, 0.1003, 0.7, 1e9, -1e9};
    const size_t NS = sizeof(special) / sizeof(special[0]);
    double acc = 0;
    for (size_t R : {1, 3}) {
        for (size_t cap : {1, 2, 7, 50}) {
            const size_t stride = cap + kSmpGuardLo + kSmpGuardHi + 3;
            for (size_t N : {1, 9, 40}) {
                for (size_t a = 0; a < NS; a++) {
                    for (size_t b = 0; b < NS; b += 3) {
                        std::vector<double> mem(R * stride + kSmpGuardLo, 0.0), in(N * R), en(N * R), out(N * R), mix(R, 0.5), st(R, special[a]), ed(R, special[b]);
                        std::vector<double> recpos(R, special[(a + b) % NS]), lag(R, 0.0), pos(R, special[(a * 3 + b) % NS]), level(R, 200.0);
                        std::vector<uint64_t> len(R);
                        std::vector<uint32_t> drop(R, 0);
                        for (size_t r = 0; r < R; r++) len[r] = 1 + (cap - 1) * (r + 1) / R;
                        for (size_t i = 0; i < N * R; i++) { in[i] = special[(i * 7 + a) % NS]; en[i] = special[(i * 5 + b) % NS]; }
                        double *pool = mem.data() + kSmpGuardLo;
                        for (size_t cut = 0; cut <= N; cut += (N > 9 ? 7 : 1)) {
                            for (int mode : {MXG_LOOPER_PLAY_NONE, 0, 2}) {
                                lp_h_render(R, cut, pool, stride, len.data(), in.data(), en.data(), 1, mix.data(), st.data(), ed.data(), recpos.data(),
                                            lag.data(), mode, st.data(), ed.data(), pos.data(), out.data(), drop.data());
                                lp_h_render(R, N - cut, pool, stride, len.data(), in.data() + cut * R, en.data(), 0, mix.data(), st.data(), ed.data(),
                                            recpos.data(), lag.data(), mode, ed.data(), st.data(), pos.data(), out.data() + cut * R, nullptr);
                            }
                        }
                        for (int piece : {1, 5, 128})
                            lp_h_render_pieces(piece, 2, R, N, pool, stride, len.data(), in.data(), en.data(), 1, mix.data(), st.data(), ed.data(),
                                               recpos.data(), lag.data(), piece == 5 ? 0 : 2, st.data(), ed.data(), pos.data(), out.data(), drop.data());
                        lp_h_normalise(R, pool, stride, len.data(), level.data());
                        for (size_t r = 0; r < R; r++) {   // the guards and the tails stay zero
                            for (long long i = -kSmpGuardLo; i < 0; i++) acc += pool[r * stride + i] != 0.0 ? 1e9 : 0.0;
                            for (size_t i = len[r]; i < cap + 6; i++) acc += pool[r * stride + i] != 0.0 ? 1e9 : 0.0;
                        }
                        acc += drop[0] & 1;
                    }
                }
            }
        }
    }
    printf("host_looper: ok (%g)\n", acc);
    return acc < 1e9 ? 0 : 1;
}
#endif
