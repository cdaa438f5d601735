// tests/host_scan_long_swept_main.cpp -- mxg_scan_long_swept.h in a stand-alone program (tests/test_scan_long_swept_host.py builds it
// with -fsanitize=address,undefined and runs it): every swept kind at a small ragged shape (3 * 1024 + 5 * 64 + 7 samples) and at 66
// chunks, three voices, coef_rows 3 and 2, a guard band round every array, two carried calls, out of place and in place, against the
// plain sequential step fed the same per-sample coefficients.  argv[1..3]: the bound of lores, hires and the lag (x the voice's peak of
// the sequential output).  Exit status 0, or 1 on a mismatch beyond the bound or a touched guard band; the sanitizers abort on
// anything they find.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mxg_scan_long_swept.h"

using namespace mxg;

namespace {

const char *const kName[3] = {"lores", "hires", "lag"};
constexpr double kGuard = 12345.678;
constexpr size_t kPad = 16;

double noise(unsigned long long &s) {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

template <int KIND>
void sequential(size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out) {
    constexpr int D = swept_dim(KIND);
    for (size_t v = 0; v < V; v++) {
        ScanStep<KIND> step = {};
        S3 s = {st[v], D == 2 ? st[V + v] : 0.0, 0.0};
        for (size_t n = 0; n < N; n++) {
            step.c[0] = coef[(n * rows) * V + v];
            step.c[1] = coef[(n * rows + 1) * V + v];
            out[n * V + v] = step(s, in[n * V + v]);
        }
        st[v] = s.a;
        if (D == 2) st[V + v] = s.b;
    }
}

struct Guarded {  // n doubles between two guard bands
    std::vector<double> a;
    explicit Guarded(size_t n) : a(n + 2 * kPad, kGuard) {}
    double *p() { return a.data() + kPad; }
    bool intact() const {
        for (size_t i = 0; i < kPad; i++)
            if (a[i] != kGuard || a[a.size() - 1 - i] != kGuard) return false;
        return true;
    }
};

template <int KIND>
int run(size_t N, size_t rows, double rtol) {
    constexpr int D = swept_dim(KIND);
    const size_t V = 3, calls = 2, C = N / kSweptChunk, NN = calls * N;
    unsigned long long seed = 3100 + KIND;
    Guarded in(NN * V), out(NN * V), ref(NN * V), coef(NN * rows * V), st(D * V), st_ref(D * V), st_ip(D * V),
        work((kSweptPairDoubles + kSweptEndDoubles) * C + 1);
    for (size_t i = 0; i < NN * V; i++) in.p()[i] = noise(seed);
    for (size_t n = 0; n < NN; n++)
        for (size_t v = 0; v < V; v++) {  // a triangle LFO per voice: lores / hires c 0.002 ... 0.6, r 0.9 ... 0.999; lag alpha 1e-6 ... 1, 1 - alpha
            const double ph = fmod((double)n / (double)(700 + 900 * v), 1.0), tri = ph < 0.5 ? 2.0 * ph : 2.0 - 2.0 * ph;
            double *c = coef.p() + (n * rows) * V + v;
            for (size_t r = 2; r < rows; r++) c[r * V] = NAN;  // (rows the scan must not read)
            if (KIND == 5) c[0] = 1e-6 + (1.0 - 1e-6) * tri * tri, c[V] = 1.0 - c[0];
            else c[0] = 0.002 + 0.598 * tri, c[V] = 0.9 + 0.099 * (1.0 - tri);
        }
    for (size_t i = 0; i < D * V; i++) st.p()[i] = st_ref.p()[i] = st_ip.p()[i] = 0.5 * noise(seed);
    for (size_t b = 0; b < calls; b++) {
        scan_long_swept_host_voices<KIND>(V, N, in.p() + b * N * V, coef.p() + b * N * rows * V, rows, st.p(), out.p() + b * N * V, work.p());
        sequential<KIND>(V, N, in.p() + b * N * V, coef.p() + b * N * rows * V, rows, st_ref.p(), ref.p() + b * N * V);
    }
    int bad = 0;
    for (size_t v = 0; v < V; v++) {
        double peak = 1e-300, err = 0.0;
        for (size_t n = 0; n < NN; n++) {
            peak = fmax(peak, fabs(ref.p()[n * V + v]));
            err = fmax(err, fabs(out.p()[n * V + v] - ref.p()[n * V + v]));
        }
        if (!(err <= rtol * peak)) bad = 1;
        printf("%-6s N=%zu rows=%zu voice %zu: |swept long - sequential| / peak = %.3e (bound %.0e)%s\n", kName[KIND - 3], N, rows, v, err / peak, rtol,
               err <= rtol * peak ? "" : "  BEYOND");
    }
    for (size_t b = 0; b < calls; b++)  // in place: the same bits
        scan_long_swept_host_voices<KIND>(V, N, in.p() + b * N * V, coef.p() + b * N * rows * V, rows, st_ip.p(), in.p() + b * N * V, work.p());
    for (size_t i = 0; i < NN * V; i++)
        if (in.p()[i] != out.p()[i]) {
            printf("%-6s N=%zu: in place differs at %zu\n", kName[KIND - 3], N, i);
            bad = 1;
            break;
        }
    for (size_t i = 0; i < D * V; i++)
        if (st_ip.p()[i] != st.p()[i]) bad = 1, printf("%-6s N=%zu: in place: state differs\n", kName[KIND - 3], N);
    if (!(in.intact() && out.intact() && coef.intact() && st.intact() && st_ip.intact() && work.intact())) bad = 1, printf("%-6s N=%zu: a guard band was written\n", kName[KIND - 3], N);
    return bad;
}

template <int KIND>
int run_shapes(double rtol) {
    return run<KIND>(3 * kSweptChunk + 5 * 64 + 7, 3, rtol) | run<KIND>(66 * (size_t)kSweptChunk, 2, rtol) | run<KIND>(63, 8, rtol);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s <bound of lores> <bound of hires> <bound of the lag>\n", argv[0]);
        return 2;
    }
    const int bad = run_shapes<3>(atof(argv[1])) | run_shapes<4>(atof(argv[2])) | run_shapes<5>(atof(argv[3]));
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
