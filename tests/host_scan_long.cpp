// tests/host_scan_long.cpp -- what tests/scan_host.py's host build lacks for the long scan's tests (tests/scan_long_host.py):
//   scan_long_lag_ld   maxiLagExp's recurrence val = (alpha * x) + (alphaReciprocal * val), sample after sample, in long double
//                      (x86-64: 64-bit mantissa): how far the float64 sequential recurrence itself is from the truth.
// coef [2][V] = alpha, alphaReciprocal; st [1][V] in and out, rounded to double; out [N][V] rounded to double once.
#include <stddef.h>

extern "C" int scan_long_lag_ld(size_t V, size_t N, const double *in, const double *coef, double *st, double *out) {
    typedef long double ld;
    for (size_t v = 0; v < V; v++) {
        const ld a = coef[v], r = coef[V + v];
        ld val = st[v];
        for (size_t n = 0; n < N; n++) {
            val = (a * (ld)in[n * V + v]) + (r * val);
            out[n * V + v] = (double)val;
        }
        st[v] = (double)val;
    }
    return 0;
}
