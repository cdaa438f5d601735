// tests/host_scan_long_main.cpp -- mxg_scan_long.h in a stand-alone program (tests/test_scan_long_host.py builds it with
// -fsanitize=address,undefined and runs it): every kind at the ragged shape (3 * 2048 + 5 * 64 + 7 samples) and at 65 chunks, three
// voices with a guard band round every array, two carried calls, out of place and in place, against the plain sequential step.
// argv[1..6]: the bound per kind (x the voice's peak of the sequential output).  Exit status 0, or 1 on a mismatch beyond the bound
// or a touched guard band; the sanitizers abort on anything they find.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mxg_scan_long.h"

using namespace mxg;

namespace {

// one stable setting per kind at 44.1 kHz: R 0.995; SVF 700 Hz, res 2, mixes 0.5 0.25 0.125 0.6; low-pass biquad 1200 Hz, Q 0.7;
// lores / hires 800 Hz, res 3; lag alpha 0.01
const double kCoef[kLongKinds][9] = {
    {0.995},
    {0.048574801209105692, 0.053423336294309766, 0.00242426754260204, 0.097149602418211384, 0.5, 0.5, 0.25, 0.125, 0.59999999999999998},
    {0.006500050695675272, 0.013000101391350544, 0.006500050695675272, -1.757281063685411, 0.78328126646811203},
    {0.012977537702960174, 0.96202700125533624},
    {0.012977537702960174, 0.96202700125533624},
    {0.01, 0.98999999999999999},
};
const char *const kName[kLongKinds] = {"dc", "svf", "biquad", "lores", "hires", "lag"};
constexpr double kGuard = 12345.678;
constexpr size_t kPad = 16;

double noise(unsigned long long &s) {  // uniform in [-1, 1)
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

template <int KIND>
void sequential(size_t V, size_t N, const double *in, const double *coef, double *st, double *out) {
    constexpr int NC = scan_long_ncoef(KIND), NS = scan_long_nstate(KIND);
    for (size_t v = 0; v < V; v++) {
        ScanStep<KIND> step;
        for (int r = 0; r < 9; r++) step.c[r] = r < NC ? coef[(size_t)r * V + v] : 0.0;
        S3 s = {st[v], NS >= 2 ? st[V + v] : 0.0, NS == 3 ? st[2 * V + v] : 0.0};
        for (size_t n = 0; n < N; n++) out[n * V + v] = step(s, in[n * V + v]);
        st[v] = s.a;
        if (NS >= 2) st[V + v] = s.b;
        if (NS == 3) st[2 * V + v] = s.c;
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
int run(size_t N, double rtol) {
    constexpr int NC = scan_long_ncoef(KIND), NS = scan_long_nstate(KIND);
    const size_t V = 3, calls = 2, C = N / kLongChunk;
    unsigned long long seed = 1000 + KIND;
    Guarded in(calls * N * V), out(calls * N * V), ref(calls * N * V), coef(NC * V), st(NS * V), st_ref(NS * V), st_ip(NS * V), work(6 * C + 1);
    for (size_t i = 0; i < calls * N * V; i++) in.p()[i] = noise(seed);
    for (int r = 0; r < NC; r++)
        for (size_t v = 0; v < V; v++) coef.p()[r * V + v] = kCoef[KIND][r];
    for (size_t i = 0; i < NS * V; i++) st.p()[i] = st_ref.p()[i] = st_ip.p()[i] = 0.5 * noise(seed);
    for (size_t b = 0; b < calls; b++) {
        scan_long_host_voices<KIND>(V, N, in.p() + b * N * V, coef.p(), st.p(), out.p() + b * N * V, work.p());
        sequential<KIND>(V, N, in.p() + b * N * V, coef.p(), st_ref.p(), ref.p() + b * N * V);
    }
    int bad = 0;
    for (size_t v = 0; v < V; v++) {
        double peak = 1e-300, err = 0.0;
        for (size_t n = 0; n < calls * N; n++) {
            peak = fmax(peak, fabs(ref.p()[n * V + v]));
            err = fmax(err, fabs(out.p()[n * V + v] - ref.p()[n * V + v]));
        }
        if (!(err <= rtol * peak)) bad = 1;
        printf("%-6s N=%zu voice %zu: |long - sequential| / peak = %.3e (bound %.0e)%s\n", kName[KIND], N, v, err / peak, rtol, err <= rtol * peak ? "" : "  BEYOND");
    }
    for (size_t b = 0; b < calls; b++)  // in place: the same bits
        scan_long_host_voices<KIND>(V, N, in.p() + b * N * V, coef.p(), st_ip.p(), in.p() + b * N * V, work.p());
    for (size_t i = 0; i < calls * N * V; i++)
        if (in.p()[i] != out.p()[i]) {
            printf("%-6s N=%zu: in place differs at %zu\n", kName[KIND], N, i);
            bad = 1;
            break;
        }
    for (size_t i = 0; i < NS * V; i++)
        if (st_ip.p()[i] != st.p()[i]) bad = 1, printf("%-6s N=%zu: in place: state differs\n", kName[KIND], N);
    if (!(in.intact() && out.intact() && coef.intact() && st.intact() && st_ip.intact() && work.intact())) bad = 1, printf("%-6s N=%zu: a guard band was written\n", kName[KIND], N);
    return bad;
}

template <int KIND>
int run_shapes(double rtol) {
    return run<KIND>(3 * kLongChunk + 5 * 64 + 7, rtol) | run<KIND>(65 * (size_t)kLongChunk, rtol);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 1 + kLongKinds) {
        fprintf(stderr, "usage: %s <bound of kind 0> ... <bound of kind 5>\n", argv[0]);
        return 2;
    }
    double rtol[kLongKinds];
    for (int k = 0; k < kLongKinds; k++) rtol[k] = atof(argv[1 + k]);
    const int bad = run_shapes<0>(rtol[0]) | run_shapes<1>(rtol[1]) | run_shapes<2>(rtol[2]) | run_shapes<3>(rtol[3]) | run_shapes<4>(rtol[4]) | run_shapes<5>(rtol[5]);
    printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
