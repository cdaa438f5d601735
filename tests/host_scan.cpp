// tests/host_scan.cpp -- host build of mxg_scan.h (tests/scan_host.py, tests/test_scan_host.py, tests/test_gpu_scan.py):
//   scan_host_render   the 64-lane model of scan.hip's kernel: the lane-exchange primitive over arrays of 64 lane values, a bank
//                      [N][V] with carried state, the layouts of scan_filter_launch.  The device must give these bits.
//   scan_host_seq_ld   the five recurrences, sample after sample, in long double (x86-64: 64-bit mantissa): the high-precision
//                      reference that says how far the float64 sequential recurrence itself is from the truth.
// kind: 0 maxiDCBlocker, 1 maxiSVF, 2 maxiBiquad, 3 lores, 4 hires; coefficient rows [NC][V] and state rows [NS][V] as the kernel's.
#include <stddef.h>

#include "mxg_scan.h"

using namespace mxg;

namespace {

struct HostXch {
    int lane(int w) const { return w; }
    void up(const double (&src)[kScanLanes], int d, double (&dst)[kScanLanes]) const {
        for (int k = 0; k < kScanLanes; k++) dst[k] = k >= d ? src[k - d] : src[k];  // (__shfl_up: lanes below d keep their own)
    }
    double from(const double (&src)[kScanLanes], int j) const { return src[j]; }
};

template <int KIND, int L>
void render(size_t V, const double *in, const double *coef, double *st, double *out) {
    constexpr int NC = scan_ncoef(KIND), NS = scan_nstate(KIND);
    for (size_t v = 0; v < V; v++) {
        ScanStep<KIND> step;
        for (int r = 0; r < 9; r++) step.c[r] = r < NC ? coef[(size_t)r * V + v] : 0.0;
        const S3 s_in = {st[v], st[V + v], NS == 3 ? st[2 * V + v] : 0.0};
        double x[kScanLanes][L];
        for (int k = 0; k < kScanLanes; k++)
            for (int i = 0; i < L; i++) x[k][i] = in[((size_t)k * L + i) * V + v];
        S3 s[kScanLanes];
        scan_voice<KIND, L, kScanLanes>(HostXch{}, step, s_in, x,
                                        [&](int w, int i, double y) { out[((size_t)w * L + i) * V + v] = y; }, s);
        st[v] = s[kScanLanes - 1].a;
        st[V + v] = s[kScanLanes - 1].b;
        if (NS == 3) st[2 * V + v] = s[kScanLanes - 1].c;
    }
}

template <int KIND>
int render_l(size_t V, size_t N, const double *in, const double *coef, double *st, double *out) {
    switch (N / kScanLanes) {
        case 1: render<KIND, 1>(V, in, coef, st, out); break;
        case 2: render<KIND, 2>(V, in, coef, st, out); break;
        case 4: render<KIND, 4>(V, in, coef, st, out); break;
        case 8: render<KIND, 8>(V, in, coef, st, out); break;
        case 16: render<KIND, 16>(V, in, coef, st, out); break;
        case 32: render<KIND, 32>(V, in, coef, st, out); break;
        default: return 1;
    }
    return 0;
}

}  // namespace

extern "C" int scan_host_render(int kind, size_t V, size_t N, const double *in, const double *coef, double *st, double *out) {
    if (N % kScanLanes) return 1;
    switch (kind) {
        case 0: return render_l<0>(V, N, in, coef, st, out);
        case 1: return render_l<1>(V, N, in, coef, st, out);
        case 2: return render_l<2>(V, N, in, coef, st, out);
        case 3: return render_l<3>(V, N, in, coef, st, out);
        case 4: return render_l<4>(V, N, in, coef, st, out);
    }
    return 1;
}

// The sequential recurrences in long double (coefficients, inputs and the start state are the doubles the kernels get; every
// product and sum after that keeps 64 bits).  out [N][V] rounded to double once; st [NS][V] in and out, rounded to double.
extern "C" int scan_host_seq_ld(int kind, size_t V, size_t N, const double *in, const double *coef, double *st, double *out) {
    typedef long double ld;
    if (kind < 0 || kind > 4) return 1;
    for (size_t v = 0; v < V; v++) {
        ld c[9];
        const int NC = scan_ncoef(kind), NS = scan_nstate(kind);
        for (int r = 0; r < NC; r++) c[r] = coef[(size_t)r * V + v];
        ld a = st[v], b = st[V + v], s2 = NS == 3 ? st[2 * V + v] : 0.0;
        for (size_t n = 0; n < N; n++) {
            const ld x = in[n * V + v];
            ld o;
            if (kind == 0) {  // a = xm1, b = ym1
                b = x - a + c[0] * b;
                a = x;
                o = b;
            } else if (kind == 1) {  // a = v0z, b = v1, s2 = v2
                const ld v1z = b, v2z = s2;
                const ld v3 = x + a - 2.0L * v2z;
                b += c[0] * v3 - c[1] * v1z;
                s2 += c[2] * v3 + c[3] * v1z;
                a = x;
                const ld high = x - c[4] * b - s2, notch = x - c[4] * b;
                o = (s2 * c[5]) + (b * c[6]) + (high * c[7]) + (notch * c[8]);
            } else if (kind == 2) {  // a = v0, b = v1, s2 = v2
                a = x - (c[3] * b) - (c[4] * s2);
                o = (c[0] * a) + (c[1] * b) + (c[2] * s2);
                s2 = b;
                b = a;
            } else {  // a = x, b = y
                a = a + (x - b) * c[0];
                b = b + a;
                a = a * c[1];
                o = kind == 3 ? b : x - b;
            }
            out[n * V + v] = (double)o;
        }
        st[v] = (double)a;
        st[V + v] = (double)b;
        if (NS == 3) st[2 * V + v] = (double)s2;
    }
    return 0;
}
