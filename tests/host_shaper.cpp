// tests/host_shaper.cpp -- host build of mxg_shaper.h (tests/test_shaper_host.py; pinned to tests/golden/shaper.npz).
// The shp_host_* functions take the arguments of mxg_shape_render / mxg_xfade_render / mxg_select_render / mxg_line_render
// (include/maxigpu.h) without the stream, on host arrays in the same layouts, and run the step functions the kernels of
// shaper.hip run, element after element.  With -DSHP_HOST_MAIN the file is a stand-alone program that plays every entry over
// small shapes, the edges of every clamp and a line that is prepared, played and prepared again (the sanitizer run).
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "mxg_shaper.h"

using namespace mxg;

extern "C" {

int shp_host_shape(int mode, size_t V, size_t N, const double *in, const double *a, const double *b, int ps, double *out) {
    for (size_t e = 0; e < N * V; e++) {
        const size_t i = ps ? e : e % V;
        const double pa = mode >= MXG_SHAPE_FASTATANDIST ? a[i] : 0.0;
        double pb = 0.0;
        if (mode == MXG_SHAPE_ASYMCLIP) pb = b[i];
        if (mode == MXG_SHAPE_ATANDIST) pb = ps ? shp_atan_norm(pa) : b[i];
        switch (mode) {
            case MXG_SHAPE_HARDCLIP: out[e] = shp_apply<MXG_SHAPE_HARDCLIP>(in[e], pa, pb); break;
            case MXG_SHAPE_SOFTCLIP: out[e] = shp_apply<MXG_SHAPE_SOFTCLIP>(in[e], pa, pb); break;
            case MXG_SHAPE_FASTATAN: out[e] = shp_apply<MXG_SHAPE_FASTATAN>(in[e], pa, pb); break;
            case MXG_SHAPE_FASTATANDIST: out[e] = shp_apply<MXG_SHAPE_FASTATANDIST>(in[e], pa, pb); break;
            case MXG_SHAPE_ATANDIST: out[e] = shp_apply<MXG_SHAPE_ATANDIST>(in[e], pa, pb); break;
            case MXG_SHAPE_ASYMCLIP: out[e] = shp_apply<MXG_SHAPE_ASYMCLIP>(in[e], pa, pb); break;
            default: return -1;
        }
    }
    return 0;
}

double shp_host_atan_norm(double shape) { return shp_atan_norm(shape); }

int shp_host_xfade(size_t C, size_t V, size_t N, const double *ch1, const double *ch2, const double *xf, int ps, double *out) {
    const size_t E = N * V;
    for (size_t e = 0; e < E; e++) {
        double g1, g2;
        shp_xfade_gains(xf[ps ? e : e % V], g1, g2);
        for (size_t c = 0; c < C; c++) out[c * E + e] = shp_xfade(ch1[c * E + e], ch2[c * E + e], g1, g2);
    }
    return 0;
}

int shp_host_select(int interpolate, size_t K, size_t V, size_t N, const double *index, const double *values, int sig, int normalised,
                    uint32_t *nan_count, double *out) {
    const size_t E = N * V, plane = sig ? E : V;
    for (size_t e = 0; e < E; e++) {
        const size_t col = sig ? e : e % V;
        bool nan;
        const double ix = shp_select_index(index[e], K, normalised != 0, &nan);
        if (nan && nan_count) nan_count[e % V]++;
        if (interpolate) {
            size_t a1, a2;
            double mix;
            shp_selectx_at(ix, K, a1, a2, mix);
            out[e] = shp_selectx_mix(values[a1 * plane + col], values[a2 * plane + col], mix);
        } else {
            out[e] = values[shp_select_at(ix) * plane + col];
        }
    }
    return 0;
}

int shp_host_line(size_t V, size_t N, const double *trig, double trig_const, const double *par, double *st, double *out) {
    for (size_t v = 0; v < V; v++) {
        const LinePar p = {par[v], par[V + v], par[2 * V + v], par[3 * V + v] != 0.0, par[4 * V + v] != 0.0};
        LineState s = {st[v], st[V + v], st[2 * V + v], st[3 * V + v] != 0.0};
        for (size_t n = 0; n < N; n++) out[n * V + v] = shp_line(s, p, trig ? trig[n * V + v] : trig_const);
        st[v] = s.value;
        st[V + v] = s.last;
        st[2 * V + v] = s.triggered;
        st[3 * V + v] = s.complete ? 1.0 : 0.0;
    }
    return 0;
}

int shp_host_line_prepare(size_t V, const double *start, const double *end, const double *ms, const int32_t *oneshot, const int32_t *mask,
                          double sr, double *par, double *st) {
    for (size_t v = 0; v < V; v++) {
        if (mask && !mask[v]) continue;
        LineState s = {st[v], st[V + v], st[2 * V + v], st[3 * V + v] != 0.0};
        LinePar p = {par[v], par[V + v], par[2 * V + v], par[3 * V + v] != 0.0, par[4 * V + v] != 0.0};
        shp_line_prepare(s, p, start[v], end[v], ms[v], oneshot[v] != 0, sr);
        st[v] = s.value; st[2 * V + v] = s.triggered; st[3 * V + v] = s.complete ? 1.0 : 0.0;
        par[v] = p.start; par[V + v] = p.end; par[2 * V + v] = p.inc; par[3 * V + v] = p.oneShot ? 1.0 : 0.0;
    }
    return 0;
}

}  // extern "C"

#ifdef SHP_HOST_MAIN
int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double special[] = {-inf, -1.5, -1.0, -0.999, -0.0, 0.0, 0.5, 1.0, 1.25, inf, nan, 1e-310, 63.999999999, 64.0, -1e-9};
    const size_t NS = sizeof(special) / sizeof(special[0]);
    double acc = 0;
    for (size_t V : {1, 3, 4}) {
        for (size_t N : {1, 7, 9}) {
            const size_t E = V * N;
            std::vector<double> x(E), a(E), b(E), o(8 * E), pv(V, 2.5), nv(V, shp_atan_norm(2.5));
            for (size_t i = 0; i < E; i++) { x[i] = special[(i * 7 + V + N) % NS]; a[i] = 0.5 + (double)(i % 11); b[i] = 0.25 + (double)(i % 5); }
            for (int mode = 0; mode < MXG_SHAPE_MODES; mode++) {
                shp_host_shape(mode, V, N, x.data(), a.data(), b.data(), 1, o.data());
                shp_host_shape(mode, V, N, x.data(), pv.data(), mode == MXG_SHAPE_ATANDIST ? nv.data() : pv.data(), 0, o.data());
                for (size_t i = 0; i < E; i++) acc += o[i] == o[i] && o[i] < 1e300 && o[i] > -1e300 ? o[i] : 0.0;
            }
            for (size_t C : {1, 2, 8}) {
                std::vector<double> c1(C * E, 0.5), c2(C * E, -0.25), oc(C * E);
                shp_host_xfade(C, V, N, c1.data(), c2.data(), x.data(), 1, oc.data());
                shp_host_xfade(C, V, N, c1.data(), c2.data(), pv.data(), 0, c1.data());  // in place
                acc += c1[C * E - 1];
            }
            for (size_t K : {1, 2, 5, 64}) {
                std::vector<double> vals(K * E), idx(E);
                std::vector<uint32_t> cnt(V, 0);
                for (size_t i = 0; i < K * E; i++) vals[i] = (double)i;
                for (size_t i = 0; i < E; i++) idx[i] = special[(i * 5 + K) % NS];
                for (int interp = 0; interp < 2; interp++)
                    for (int norm = 0; norm < 2; norm++) {
                        shp_host_select(interp, K, V, N, idx.data(), vals.data(), 1, norm, cnt.data(), o.data());
                        shp_host_select(interp, K, V, N, idx.data(), vals.data(), 0, norm, nullptr, o.data());
                    }
                acc += cnt[0];
            }
            std::vector<double> par(5 * V, 0.0), st(4 * V, 0.0), st0(V), en(V), ms(V), trig(E);
            std::vector<int32_t> one(V), mask(V, 1);
            for (size_t v = 0; v < V; v++) { par[3 * V + v] = 1.0; par[4 * V + v] = v != 1; st[V + v] = -1.0; st0[v] = (double)v; en[v] = v & 1 ? -2.0 : 2.0; ms[v] = v == 2 ? 0.0 : 3.0; one[v] = v & 1; }
            for (size_t i = 0; i < E; i++) trig[i] = (i / V) % 3 == 0 ? 1.0 : -1.0;
            for (int rep = 0; rep < 3; rep++) {
                shp_host_line_prepare(V, st0.data(), en.data(), ms.data(), one.data(), rep ? mask.data() : nullptr, 1000.0, par.data(), st.data());
                shp_host_line(V, N, trig.data(), 0.0, par.data(), st.data(), o.data());
                shp_host_line(V, N, nullptr, 1.0, par.data(), st.data(), o.data());
                mask[0] = 0;
            }
            acc += st[0];
        }
    }
    printf("host_shaper: ok (%g)\n", acc);
    return 0;
}
#endif
