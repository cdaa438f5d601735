// mxg_kuramoto.h -- maxiKuramotoOscillator::play (H:1640-1654), maxiKuramotoOscillatorSet::play (H:1714-1727) and
// maxiAsyncKuramotoOscillator::play (H:1775-1792) as plain arithmetic over one set's phases.  H = src/maximilian.h.  No device
// state: the same text compiles for the host (tests/host_kuramoto.cpp, tests/host_kuramoto_wide.cpp) and for the kernels K17
// (kuramoto.hip: sets of up to 64, several to a wavefront) and K26 (kuramoto_wide.hip: up to 1024, a workgroup each), and host
// and device agree bit for bit.
//
// Per set and sample the reference gathers phases[j] = oscs[j].phase, then for every oscillator i, in order,
//     adj = 0; for j: adj += sin(phases[j] - phase_i);                      (sequential in j)
//     phase_i += dt * (freq + ((K / (double)N) * adj));
//     if (phase_i >= TWOPI) phase_i -= TWOPI; else if (phase_i < 0) phase_i += TWOPI;     (ONE wrap)
// and returns (sum of the new phases in i order, from 0.0) / (double)N.  Every oscillator reads the phases gathered before any
// of them moved.  The async class refreshes the gathered phases only when its flag is up, plays with K when it is up and with 0
// otherwise (the sum is still formed and multiplied by 0 / N, so a non-finite phase propagates), and clears the flag.
//
// Everything except sin() keeps the reference's expression trees and orders (-ffp-contract=off).  Two forms of the sum:
//   * exact (default): the N sines of every oscillator, summed in j order.  The one departure is the sine itself: kura_sin, at
//     most 1 ULP from glibc's per term.
//   * mean field (MXG_KURA_MEANFIELD, a TOLERANCE mode): sum_j sin(t_j - t_i) = cos t_i * S - sin t_i * C with S = sum_j sin t_j,
//     C = sum_j cos t_j, both summed in j order from 0.0 -- N sine / cosine pairs per sample instead of N * N sines.  The update
//     line, the wrap and the mix are unchanged.
//
// kura_sin / kura_cos are mxg::sin_small / cos_small (mxg_sincos.h: Cody-Waite reduction by pi/2, the fdlibm kernels, the
// accurate reduction next to a zero) with every fused multiply-add SPELLED as fma().  sin_small leaves the fusing to the device
// compiler (#pragma clang fp contract(fast)), which a host compiler reads differently; spelled out, the expression tree is one
// and the same on both sides and fma() is exact, so the host build IS the device's arithmetic.  Same constants, same error
// bound (< 0.85 ULP; tests/host_kuramoto.cpp measures it against long double).  Two refinements that change no result:
//   * the accurate reduction is skipped where k = 0 (|x| < pi/4): there the one-shot reduction is y = x, t = 0 exactly, and so is
//     the accurate one.  A set in sync has all its differences there; the term j = i (x = 0) always is.
//   * over a group of U terms the "some remainder is small" test is ONE branch (wave-uniform on the device), so that the U
//     chains between two branches are independent and the rare path stays out of every term.
// |x| > 64, NaN, Inf go to the platform's sin()/cos(): such a term is within 1 ULP but not bit-identical between host and device
// (NaN and Inf give NaN on both).  A caller that keeps its phases in [0, 2 pi) -- what the wrap does for |dt * (...)| < 2 pi --
// never gets there.
#pragma once
#include <math.h>
#include <stdint.h>

#include "mxg_hd.h"
#include "mxg_sincos.h"

#define MXG_KURA_MEANFIELD 1
#define MXG_KURA_ASYNC 2
#define MXG_KURA_WANT_MIX 1
#define MXG_KURA_WANT_PHASES 2
#define MXG_KURA_MAX_N 64
#define MXG_KURA_WIDE_MAX_N 1024  // kuramoto_wide.hip (K26): one workgroup per set

namespace mxg {
namespace {

constexpr int kKuraUnroll = 4;       // independent sine chains between two branches of the exact form
constexpr double kKuraTrust = 32.0;  // all |phase| <= 32: every difference is inside the branch-free domain |x| <= 64

// ---- sine and cosine, every fused operation spelled ----------------------------------------------------------------------
struct KuraRed {
    double y, t, fn;
};
MXG_DEV KuraRed kura_reduce(double x) {
    using namespace sincos_detail;
    KuraRed r;
    r.fn = rint(x * kInvPio2);
    const double z = fma(-r.fn, kPio2Hi, x);  // exact: fn has <= 6 bits, kPio2Hi 33
    const double w = r.fn * kPio2Lo;
    r.y = z - w;
    r.t = fma(-r.fn, kPio2Lo2, (z - r.y) - w);
    return r;
}
MXG_DEV bool kura_rare(const KuraRed &r) { return fabs(r.y) < sincos_detail::kSmallRem && r.fn != 0.0; }
MXG_DEV double kura_ksin(double y, double t) {
    using namespace sincos_detail;
    const double z = y * y, v = z * y;
    const double r = fma_k(z, fma_k(z, fma_k(z, fma_kk(z, S6, S5), S4), sincos_detail::S3), S2);  // (S3 qualified: mxg_scan.h has a struct of that name)
    return y - fma(-v, S1, fma(z, fma(-v, r, 0.5 * t), -t));
}
MXG_DEV double kura_kcos(double y, double t) {
    using namespace sincos_detail;
    const double z = y * y;
    const double r = z * fma_k(z, fma_k(z, fma_k(z, fma_k(z, fma_kk(z, C6, C5), C4), C3), C2), C1);
    const double hz = 0.5 * z, w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + fma(z, r, -(y * t)));
}
MXG_DEV double kura_sin_of(const KuraRed &r) {
    const int n = (int)r.fn;
    const double s = kura_ksin(r.y, r.t), c = kura_kcos(r.y, r.t);
    const double v = (n & 1) ? c : s;
    return (n & 2) ? -v : v;
}
MXG_DEV double kura_cos_of(const KuraRed &r) {
    const int n = (int)r.fn;
    const double s = kura_ksin(r.y, r.t), c = kura_kcos(r.y, r.t);
    const double v = (n & 1) ? s : c;
    return ((n + 1) & 2) ? -v : v;
}
// the reduction of ONE argument that is known to lie in |x| <= 64
MXG_DEV KuraRed kura_reduce_full(double x) {
    KuraRed r = kura_reduce(x);
    if (kura_rare(r)) sincos_detail::reduce_accurate(x, r.y, r.t);
    return r;
}
// any argument
MXG_DEV double kura_sin(double x) {
    if (!(fabs(x) <= 64.0)) return sin(x);
    return kura_sin_of(kura_reduce_full(x));
}
MXG_DEV double kura_cos(double x) {
    if (!(fabs(x) <= 64.0)) return cos(x);
    return kura_cos_of(kura_reduce_full(x));
}

// true on every lane when `c` holds on some lane of the wavefront; the host has one lane
MXG_DEV bool kura_any(bool c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(c) != 0;
#else
    return c;
#endif
}

// U sines of arguments in |x| <= 64, the rare accurate reduction behind one branch for all of them
template <int U>
MXG_DEV void kura_sin_group(const double (&x)[U], double (&s)[U]) {
    KuraRed r[U];
    bool rare = false;
#pragma unroll
    for (int u = 0; u < U; u++) {
        r[u] = kura_reduce(x[u]);
        rare |= kura_rare(r[u]);
    }
    if (kura_any(rare)) {
#pragma unroll
        for (int u = 0; u < U; u++)
            if (kura_rare(r[u])) sincos_detail::reduce_accurate(x[u], r[u].y, r[u].t);
    }
#pragma unroll
    for (int u = 0; u < U; u++) s[u] = kura_sin_of(r[u]);
}

// ---- maxiKuramotoOscillator::play: the sum over the gathered phases ----------------------------------------------------
// TRUST: every g[j] - phase lies in |x| <= 64 (all |phases| <= kKuraTrust).  Same bits either way inside that domain.
template <bool TRUST>
MXG_DEV double kura_adj_exact(const double *g, int N, double phase) {
    double adj = 0;
    if constexpr (TRUST) {
        constexpr int U = kKuraUnroll;
        int j = 0;
        for (; j + U <= N; j += U) {
            double x[U], s[U];
#pragma unroll
            for (int u = 0; u < U; u++) x[u] = g[j + u] - phase;
            kura_sin_group<U>(x, s);
#pragma unroll
            for (int u = 0; u < U; u++) adj += s[u];
        }
        for (; j < N; j++) adj += kura_sin_of(kura_reduce_full(g[j] - phase));
    } else {
        for (int j = 0; j < N; j++) adj += kura_sin(g[j] - phase);
    }
    return adj;
}

// mean field: one oscillator's sine and cosine ...
template <bool TRUST>
MXG_DEV void kura_sincos(double phase, double &s, double &c) {
    if (!TRUST && !(fabs(phase) <= 64.0)) {
        s = sin(phase);
        c = cos(phase);
        return;
    }
    const KuraRed r = kura_reduce_full(phase);
    const int n = (int)r.fn;
    const double ks = kura_ksin(r.y, r.t), kc = kura_kcos(r.y, r.t);
    const double vs = (n & 1) ? kc : ks, vc = (n & 1) ? ks : kc;
    s = (n & 2) ? -vs : vs;
    c = ((n + 1) & 2) ? -vc : vc;
}
// ... and the sum from the set's sines and cosines: cos t_i * S - sin t_i * C, S and C in j order from 0.0
MXG_DEV double kura_adj_meanfield(const double *sj, const double *cj, int N, double si, double ci) {
    double S = 0.0, C = 0.0;
    for (int j = 0; j < N; j++) {
        S += sj[j];
        C += cj[j];
    }
    return ci * S - si * C;
}

// The same sum in two steps, for a kernel in which one lane forms S and C and every lane of the set reads them (kernel K26):
// exactly what kura_adj_meanfield gives -- j order, from 0.0.
MXG_DEV void kura_meanfield_sums(const double *sj, const double *cj, int N, double &S, double &C) {
    S = 0.0;
    C = 0.0;
    for (int j = 0; j < N; j++) {
        S += sj[j];
        C += cj[j];
    }
}
MXG_DEV double kura_meanfield_adj(double si, double ci, double S, double C) { return ci * S - si * C; }

// the update line and the one wrap; returns what the oscillator's play() returns
MXG_DEV double kura_advance(double phase, double dt, double freq, double K, int N, double adj) {
    phase += dt * (freq + ((K / (double)N) * adj));
    if (phase >= MXG_TWOPI) phase -= MXG_TWOPI;
    else if (phase < 0) phase += MXG_TWOPI;
    return phase;
}

// maxiKuramotoOscillatorSet::play's return value from the new phases
MXG_DEV double kura_mix(const double *p, int N) {
    double mix = 0.0;
    for (int i = 0; i < N; i++) mix += p[i];
    return mix / (double)N;
}

// Where K is forced to 0 (an async set whose flag is down) the sum may be left out when the result is provably the same:
// all arguments finite (here: inside the trusted domain) makes (0.0 / N) * adj a zero of either sign, and freq + (+-0.0) is
// freq bit for bit unless freq is -0.0.
MXG_DEV bool kura_zero_k_skippable(bool trusted, double freq) { return trusted && !(freq == 0.0 && signbit(freq)); }

}  // namespace
}  // namespace mxg
