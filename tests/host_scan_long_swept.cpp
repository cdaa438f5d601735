// tests/host_scan_long_swept.cpp -- the swept recurrences of K31's kinds in long double (x86-64: 64-bit mantissa), sample after
// sample, from the float64 coefficients of every sample: how far the float64 sequential recurrence itself is from the truth
// (tests/scan_long_swept_host.py, tools/measure_longsweep_tolerance.py).
//   kind 3 lores, 4 hires: x = x + (in - y) * c; y = y + x; x = x * r; out = y (lores) or in - y (hires)   (maxiFilter, C:455-484)
//   kind 5 maxiLagExp:     val = (alpha * in) + (alphaReciprocal * val)                                      (H:523-556)
// coef [N][rows][V], rows 0-1 read; st [2][V] or [1][V] in and out, rounded to double; out [N][V] rounded to double once.
#include <stddef.h>

extern "C" int scan_long_swept_ld(int kind, size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out) {
    typedef long double ld;
    if (kind < 3 || kind > 5 || rows < 2) return 1;
    for (size_t v = 0; v < V; v++) {
        ld a = st[v], b = kind == 5 ? 0.0L : (ld)st[V + v];
        for (size_t n = 0; n < N; n++) {
            const ld x = in[n * V + v], c0 = coef[(n * rows) * V + v], c1 = coef[(n * rows + 1) * V + v];
            if (kind == 5) {
                a = (c0 * x) + (c1 * a);
                out[n * V + v] = (double)a;
            } else {
                a = a + (x - b) * c0;
                b = b + a;
                a = a * c1;
                out[n * V + v] = (double)(kind == 3 ? b : x - b);
            }
        }
        st[v] = (double)a;
        if (kind != 5) st[V + v] = (double)b;
    }
    return 0;
}
