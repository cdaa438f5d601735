// tests/host_classic.cpp -- host build of mxg_classic.h (tests/test_classic_host.py; pinned to tests/golden/classic.npz).
// The cls_h_* functions take the arguments of mxg_dyn_gate_render / mxg_dyn_compress_render / mxg_envelope_line_render /
// mxg_lag_render / mxg_map_render (include/maxigpu.h) without the stream (the line: with the sample rate), on host arrays in the
// same layouts, and run the step functions the kernels of classic.hip run, voice after voice.  With -DCLS_HOST_MAIN the file is
// a stand-alone program that plays every entry over small shapes, every special value, tables of every legal and illegal count
// and start index, and blocks cut at every position (the sanitizer run).
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "mxg_classic.h"

using namespace mxg;

extern "C" {

int cls_h_gate(size_t V, size_t N, const double *in, const double *thr, const double *att, const double *rel, int ps, const int64_t *holdtime,
               double *dst, int64_t *ist, double *out) {
    cls_host_gate(V, N, in, thr, att, rel, ps, holdtime, dst, ist, out);
    return 0;
}

int cls_h_compress(size_t V, size_t N, const double *in, const double *ratio, const double *makeup, const double *thr, const double *att,
                   const double *rel, int ps, double *dst, int64_t *ist, double *out) {
    cls_host_compress(V, N, in, ratio, makeup, thr, att, rel, ps, dst, ist, out);
    return 0;
}

int cls_h_line(size_t V, size_t N, size_t S, const double *seg, const int32_t *count, const double *trig, const int32_t *trig_index,
               const double *trig_amp, double sr, double *dst, int32_t *ist, double *out) {
    cls_host_line(V, N, S, seg, count, trig, trig_index, trig_amp, sr, dst, ist, out);
    return 0;
}

int cls_h_lag(size_t V, size_t N, const double *in, const double *alpha, const double *recip, int ps, double *val, double *out) {
    cls_host_lag(V, N, in, alpha, recip, ps, val, out);
    return 0;
}

int cls_h_map(int mode, size_t V, size_t N, const double *in, const double *range, const double *aux, double *out) {
    return cls_host_map(mode, V, N, in, range, aux, out);
}

double cls_h_makeup(double ratio) { return cls_makeup(ratio); }
double cls_h_coeff(double ms, double sr) { return cls_dyn_coeff(ms, sr); }
double cls_h_explin_den(double inMin, double inMax) { return cls_explin_den(inMin, inMax); }

}  // extern "C"

#ifdef CLS_HOST_MAIN
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double special[] = {-inf, -1.5, -1.0, -0.999, -0.0, 0.0, 0.5, 1.0, 1.25, inf, nan, 1e-310, 0.95, 0.05, -1e-9, 3.0};
    const size_t NS = sizeof(special) / sizeof(special[0]);
    double acc = 0;
    for (size_t V : {1, 3, 4}) {
        for (size_t N : {1, 7, 9, 40}) {
            const size_t E = V * N;
            std::vector<double> x(E), o(E), pv(V), ps(E), thr(V, 0.4), rat(V), mk(V), ratps(E), mkps(E);
            for (size_t i = 0; i < E; i++) { x[i] = special[(i * 7 + V + N) % NS]; ps[i] = special[(i * 3 + 1) % NS]; ratps[i] = 0.5 + (double)(i % 7); mkps[i] = cls_makeup(ratps[i]); }
            for (size_t v = 0; v < V; v++) { pv[v] = 0.25 * (double)(v + 1); rat[v] = v & 1 ? 0.75 : 5.0; mk[v] = cls_makeup(rat[v]); }
            // dynamics: per voice, every parameter per sample (special values as parameters too), cut at every position
            for (int flags : {0, 1, 2, 4, 7, 8, 15}) {
                std::vector<double> dst(3 * V, 0.0);
                std::vector<int64_t> ist(4 * V, 0), hold(V);
                for (size_t v = 0; v < V; v++) hold[v] = (int64_t)v * 3;
                for (size_t cut = 0; cut <= N; cut += (N > 9 ? 7 : 1)) {
                    const double *t = (flags & 1) ? ps.data() : thr.data(), *a = (flags & 2) ? ps.data() : pv.data(), *r = (flags & 4) ? ps.data() : pv.data();
                    if (!(flags & 8)) {
                        cls_h_gate(V, cut, x.data(), t, a, r, flags, hold.data(), dst.data(), ist.data(), o.data());
                        cls_h_gate(V, N - cut, x.data() + cut * V, t + (flags & 1 ? cut * V : 0), a + (flags & 2 ? cut * V : 0), r + (flags & 4 ? cut * V : 0),
                                   flags, hold.data(), dst.data(), ist.data(), o.data() + cut * V);
                    }
                    const double *q = (flags & 8) ? ratps.data() : rat.data(), *m = (flags & 8) ? mkps.data() : mk.data();
                    cls_h_compress(V, cut, x.data(), q, m, t, a, r, flags, dst.data(), ist.data(), o.data());
                    cls_h_compress(V, N - cut, x.data() + cut * V, q + (flags & 8 ? cut * V : 0), m + (flags & 8 ? cut * V : 0), t + (flags & 1 ? cut * V : 0),
                                   a + (flags & 2 ? cut * V : 0), r + (flags & 4 ? cut * V : 0), flags, dst.data(), ist.data(), o.data() + cut * V);
                }
                acc += (double)ist[0] + (dst[0] == dst[0] ? 1.0 : 0.0);
            }
            // the envelope: tables of S entries exactly, counts and start indices inside and outside what is legal
            for (size_t S : {2, 3, 6, 64}) {
                std::vector<double> seg(S * V), amp(V, 0.25), trig(E);
                for (size_t i = 0; i < S * V; i++) seg[i] = (i / V) & 1 ? (double)((i * 5) % 4) : special[(i * 3) % NS];
                for (size_t i = 0; i < E; i++) trig[i] = (i % 11 == 3) ? 1.0 : ((i % 17 == 5) ? nan : 0.0);
                for (int32_t cnt : {-3, 0, 1, 2, (int32_t)S - 1, (int32_t)S, (int32_t)S + 5, 1000000}) {
                    for (int32_t idx : {-7, -1, 0, 1, (int32_t)S - 2, (int32_t)S - 1, (int32_t)S, 2147483640}) {
                        std::vector<int32_t> count(V, cnt), tix(V, idx), ist(2 * V, 0);
                        std::vector<double> dst(2 * V, 0.0);
                        for (size_t v = 0; v < V; v++) { ist[v] = idx; ist[V + v] = v != 1; }   // a stored valindex anywhere
                        cls_h_line(V, N, S, seg.data(), count.data(), trig.data(), tix.data(), amp.data(), 1000.0, dst.data(), ist.data(), o.data());
                        cls_h_line(V, N, S, seg.data(), count.data(), nullptr, nullptr, nullptr, 48000.0, dst.data(), ist.data(), o.data());
                        acc += ist[0] & 1;
                    }
                }
            }
            std::vector<double> val(V, 0.5);
            cls_h_lag(V, N, x.data(), pv.data(), thr.data(), 0, val.data(), o.data());
            cls_h_lag(V, N, x.data(), ps.data(), ps.data(), 1, val.data(), o.data());
            std::vector<double> range(4 * V), aux(V);
            for (size_t v = 0; v < V; v++) { range[v] = special[(v * 5) % NS]; range[V + v] = special[(v * 3 + 2) % NS]; range[2 * V + v] = 20.0; range[3 * V + v] = v & 1 ? -5.0 : 2000.0; aux[v] = cls_h_explin_den(range[v], range[V + v]); }
            for (int mode = 0; mode < MXG_MAP_MODES; mode++) {
                cls_h_map(mode, V, N, x.data(), range.data(), aux.data(), o.data());
                std::vector<double> y(x);
                cls_h_map(mode, V, N, y.data(), range.data(), aux.data(), y.data());  // in place
                for (size_t i = 0; i < E; i++) acc += o[i] == o[i] && o[i] < 1e300 && o[i] > -1e300 ? o[i] : 0.0;
            }
        }
    }
    printf("host_classic: ok (%g)\n", acc);
    return 0;
}
#endif
