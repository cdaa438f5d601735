// tools/gen/shaper_ref_dump.cpp -- TEST INFRASTRUCTURE (never shipped).  The project's own harness around the reference's
// maxiNonlinearity, maxiXFade, maxiSelect, maxiSelectX and maxiLine: tools/gen/gen_golden_shaper.py compiles it, together with
// the UNMODIFIED reference sources, into a shared library in a temporary directory and drives it block by block to write
// tests/golden/shaper.npz.
//
// The stateless classes are called element by element on flat arrays (the caller spreads per-voice parameters over the block).
// V maxiLine objects live side by side and are called sample-major; their state is read through -fno-access-control, in the
// layouts of include/maxigpu.h (d_par [5][V], d_st [4][V]).
#include <cstdint>
#include <vector>

#include "maximilian.h"

extern "C" {

void shp_set_rate(int sr) { maxiSettings::sampleRate = sr; }

// mode: include/maxigpu.h MXG_SHAPE_*; pa = shape / a, pb = b, both [n]
void shp_shape(int mode, size_t n, const double *x, const double *pa, const double *pb, double *out) {
    maxiNonlinearity f;
    for (size_t i = 0; i < n; i++) switch (mode) {
            case 0: out[i] = f.hardclip(x[i]); break;
            case 1: out[i] = f.softclip(x[i]); break;
            case 2: out[i] = f.fastatan(x[i]); break;
            case 3: out[i] = f.fastAtanDist(x[i], pa[i]); break;
            case 4: out[i] = f.atanDist(x[i], pa[i]); break;
            default: out[i] = f.asymclip(x[i], pa[i], pb[i]); break;
        }
}

// ch1, ch2, out [C][n]; xf [n].  C == 1 goes through the mono overload, C > 1 through the vector one.
void shp_xfade(size_t C, size_t n, const double *ch1, const double *ch2, const double *xf, double *out) {
    for (size_t i = 0; i < n; i++) {
        if (C == 1) {
            out[i] = maxiXFade::xfade(ch1[i], ch2[i], xf[i]);
        } else {
            std::vector<double> a(C), b(C);
            for (size_t c = 0; c < C; c++) { a[c] = ch1[c * n + i]; b[c] = ch2[c * n + i]; }
            const std::vector<double> o = maxiXFade::xfade(a, b, xf[i]);
            for (size_t c = 0; c < C; c++) out[c * n + i] = o[c];
        }
    }
}

// values [K][n]; index [n]
void shp_select(int interpolate, size_t K, size_t n, const double *index, const double *values, int normalised, double *out) {
    maxiSelect s;
    maxiSelectX sx;
    std::vector<double> v(K);
    for (size_t i = 0; i < n; i++) {
        for (size_t k = 0; k < K; k++) v[k] = values[k * n + i];
        out[i] = interpolate ? sx.play(index[i], v, normalised != 0) : s.play(index[i], v, normalised != 0);
    }
}

void *shp_line_new(size_t V) { return new std::vector<maxiLine>(V); }
void shp_line_free(void *h) { delete (std::vector<maxiLine> *)h; }
void shp_line_prepare(void *h, size_t v, double start, double end, double ms, int oneshot) {
    (*(std::vector<maxiLine> *)h)[v].prepare(start, end, ms, oneshot != 0);
}
void shp_line_enable(void *h, size_t v, double on) { (*(std::vector<maxiLine> *)h)[v].triggerEnable(on); }

// trig [N][V] or, when null, trig_const; out, triggered, complete [N][V] (the two flags after each call, for the generator's checks)
void shp_line_play(void *h, size_t N, const double *trig, double trig_const, double *out, double *triggered, double *complete) {
    std::vector<maxiLine> &L = *(std::vector<maxiLine> *)h;
    const size_t V = L.size();
    for (size_t n = 0; n < N; n++)
        for (size_t v = 0; v < V; v++) {
            out[n * V + v] = L[v].play(trig ? trig[n * V + v] : trig_const);
            triggered[n * V + v] = L[v].triggered;
            complete[n * V + v] = L[v].isLineComplete() ? 1.0 : 0.0;
        }
}

// par [5][V] = lineStart, lineEnd, inc, oneShot, trigEnable; st [4][V] = lineValue, lastTrigVal, triggered, lineComplete
void shp_line_state(void *h, double *par, double *st) {
    std::vector<maxiLine> &L = *(std::vector<maxiLine> *)h;
    const size_t V = L.size();
    for (size_t v = 0; v < V; v++) {
        par[v] = L[v].lineStart;
        par[V + v] = L[v].lineEnd;
        par[2 * V + v] = L[v].inc;
        par[3 * V + v] = L[v].oneShot ? 1.0 : 0.0;
        par[4 * V + v] = L[v].trigEnable != 0 ? 1.0 : 0.0;
        st[v] = L[v].lineValue;
        st[V + v] = L[v].lastTrigVal;
        st[2 * V + v] = L[v].triggered != 0 ? 1.0 : 0.0;
        st[3 * V + v] = L[v].lineComplete ? 1.0 : 0.0;
    }
}

}  // extern "C"
