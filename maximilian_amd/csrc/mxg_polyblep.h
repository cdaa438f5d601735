// mxg_polyblep.h -- maxiPolyBLEP (src/libs/maxiPolyBLEP.h:47-50 over src/libs/PolyBLEP/PolyBLEP.cpp) as plain per-sample arithmetic: the
// two correction polynomials blep / blamp (P:43-64), get / inc with the "frequency >= sampleRate / 4 -> sine" fallback (P:114-160)
// and the fourteen waveforms (P:162-388).  P = PolyBLEP.cpp.  No device state: the same text compiles for the host
// (mxg_polyblep_host, tests/host_polyblep.cpp) and for the kernel of polyblep.hip (K20).  The reference's expression trees, never
// contracted into an FMA: t / dt stays a division, (-1 / 3.0 * sq) * t keeps its association, and the multiplication by
// `amplitude` (always 1.0: maxiPolyBLEP has no setter for it) is kept because 1.0 * y is exact.
//
// One call play(freq) is setFrequency (dt = freq / sr), get() on the phase t, then inc(): t += dt; t -= (int64)t.
//   * The cast truncates toward zero, so (double)(int64)x == trunc(x) for |x| < 2^63 and t - trunc(t) is exact.
//   * The fallback test is (freq / sr) * sr >= sr / 4 with the rounding of the quotient and of the product back.
//   * DOMAIN: finite frequencies with |freq / sr| < 2^62 and a finite pulse width.  NaN, Inf and anything beyond is outside the
//     contract (the reference's cast is undefined there).  A NEGATIVE frequency is inside: t then lives in (-1, 1) and every
//     waveform is evaluated on it as written.
//   * The phase never sees a transcendental: bit-exact always.  TRIANGLE, SQUARE, RECTANGLE, SAWTOOTH, RAMP, MODIFIED_TRIANGLE,
//     MODIFIED_SQUARE, TRIANGULAR_PULSE, TRAPEZOID_FIXED, TRAPEZOID_VARIABLE use + - * /, compares and fmin / fmax only:
//     bit-exact wherever the fallback is not taken.
//   * SINE, COSINE, HALF_WAVE_RECTIFIED_SINE and the fallback take sin / cos of fl(TWO_PI * t), FULL_WAVE_RECTIFIED_SINE
//     sin(fl(M_PI * t')): the caller's sine provider SC (sin(x), cos(x) of the ROUNDED product, as maxiOsc::sinewave does) --
//     PbSinTab below is mxg_sincos.h's table form, whose arguments here stay within |x| < 2 pi.  Tolerances: DESIGN.md section 4.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "mxg_hd.h"
#include "mxg_sincos.h"

// the reference's enum order (PolyBLEP.h, enum Waveform); include/maxigpu.h, where it is included, comes first and has them as an enum
#ifndef MXG_PBLEP_WAVEFORMS
#define MXG_PBLEP_SINE 0
#define MXG_PBLEP_COSINE 1
#define MXG_PBLEP_TRIANGLE 2
#define MXG_PBLEP_SQUARE 3
#define MXG_PBLEP_RECTANGLE 4
#define MXG_PBLEP_SAWTOOTH 5
#define MXG_PBLEP_RAMP 6
#define MXG_PBLEP_MODIFIED_TRIANGLE 7
#define MXG_PBLEP_MODIFIED_SQUARE 8
#define MXG_PBLEP_HALF_WAVE_RECTIFIED_SINE 9
#define MXG_PBLEP_FULL_WAVE_RECTIFIED_SINE 10
#define MXG_PBLEP_TRIANGULAR_PULSE 11
#define MXG_PBLEP_TRAPEZOID_FIXED 12
#define MXG_PBLEP_TRAPEZOID_VARIABLE 13
#define MXG_PBLEP_WAVEFORMS 14
#endif

namespace mxg {
namespace {

constexpr double kPbPi = 3.14159265358979323846;  // M_PI
constexpr double kPbTwoPi = 2 * kPbPi;            // P:32
constexpr double kPbAmp = 1.0;                    // PolyBLEP::amplitude

// sin / cos of a rounded argument through mxg_sincos.h's table (tab: MXG_SINTAB_LEN doubles, in LDS on the device)
struct PbSinTab {
    const double *tab;
    SinTabK k;
    MXG_HD double sin(double x) const { return sincos_tab<false>(x, tab, k); }
    MXG_HD double cos(double x) const { return sincos_tab<true>(x, tab, k); }
};

MXG_HD double pb_sq(double x) { return x * x; }

// x -= (int64)x
MXG_HD double pb_frac(double x) { return x - trunc(x); }

// P:43-51
MXG_HD double pb_blep(double t, double dt) {
    if (t < dt) return -pb_sq(t / dt - 1);
    if (t > 1 - dt) return pb_sq((t - 1) / dt + 1);
    return 0;
}

// P:54-64
MXG_HD double pb_blamp(double t, double dt) {
    if (t < dt) {
        t = t / dt - 1;
        return ((-1 / 3.0) * pb_sq(t)) * t;
    }
    if (t > 1 - dt) {
        t = (t - 1) / dt + 1;
        return ((1 / 3.0) * pb_sq(t)) * t;
    }
    return 0;
}

// the triangle shared by tri / trap / trap2: y = 4 t folded at 1 and 3
MXG_HD double pb_fold4(double t) {
    double y = t * 4;
    if (y >= 3) y -= 4;
    else if (y > 1) y = 2 - y;
    return y;
}

// the fallback and SINE (P:162-164)
template <class SC>
MXG_HD double pb_sin(double t, const SC &sc) { return kPbAmp * sc.sin(kPbTwoPi * t); }

// One waveform's get() below the fallback: t the phase, dt = freq / sr, pw the pulse width.
template <int WF, class SC>
MXG_HD double pb_wave(double t, double dt, double pw, const SC &sc) {
    if constexpr (WF == MXG_PBLEP_SINE) {
        return pb_sin(t, sc);
    } else if constexpr (WF == MXG_PBLEP_COSINE) {  // P:166-168
        return kPbAmp * sc.cos(kPbTwoPi * t);
    } else if constexpr (WF == MXG_PBLEP_TRIANGLE) {  // P:190-208
        const double t1 = pb_frac(t + 0.25), t2 = pb_frac(t + 0.75);
        double y = pb_fold4(t);
        y += (4 * dt) * (pb_blamp(t1, dt) - pb_blamp(t2, dt));
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_SQUARE) {  // P:320-328
        const double t2 = pb_frac(t + 0.5);
        double y = t < 0.5 ? 1 : -1;
        y += pb_blep(t, dt) - pb_blep(t2, dt);
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_RECTANGLE) {  // P:356-368
        const double t2 = pb_frac((t + 1) - pw);
        double y = -2 * pw;
        if (t < pw) y += 2;
        y += pb_blep(t, dt) - pb_blep(t2, dt);
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_SAWTOOTH) {  // P:370-378
        const double u = pb_frac(t + 0.5);
        double y = 2 * u - 1;
        y -= pb_blep(u, dt);
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_RAMP) {  // P:380-388
        const double u = pb_frac(t);
        double y = 1 - 2 * u;
        y += pb_blep(u, dt);
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_MODIFIED_TRIANGLE) {  // P:210-232
        const double w = fmax(0.0001, fmin(0.9999, pw));
        const double t1 = pb_frac(t + 0.5 * w), t2 = pb_frac((t + 1) - 0.5 * w);
        double y = t * 2;
        if (y >= 2 - w) y = (y - 2) / w;
        else if (y >= w) y = 1 - (y - w) / (1 - w);
        else y /= w;
        y += (dt / (w - w * w)) * (pb_blamp(t1, dt) - pb_blamp(t2, dt));
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_MODIFIED_SQUARE) {  // P:330-354
        double t1 = pb_frac((t + 0.875) + 0.25 * (pw - 0.5));
        double t2 = pb_frac((t + 0.375) + 0.25 * (pw - 0.5));
        double y = t1 < 0.5 ? 1 : -1;
        y += pb_blep(t1, dt) - pb_blep(t2, dt);
        t1 = pb_frac(t1 + 0.5 * (1 - pw));
        t2 = pb_frac(t2 + 0.5 * (1 - pw));
        y += t1 < 0.5 ? 1 : -1;
        y += pb_blep(t1, dt) - pb_blep(t2, dt);
        return (kPbAmp * 0.5) * y;
    } else if constexpr (WF == MXG_PBLEP_HALF_WAVE_RECTIFIED_SINE) {  // P:170-178
        const double t2 = pb_frac(t + 0.5);
        double y = t < 0.5 ? 2 * sc.sin(kPbTwoPi * t) - 2 / kPbPi : -2 / kPbPi;
        y += (kPbTwoPi * dt) * (pb_blamp(t, dt) + pb_blamp(t2, dt));
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_FULL_WAVE_RECTIFIED_SINE) {  // P:180-188
        const double u = pb_frac(t + 0.25);
        double y = 2 * sc.sin(kPbPi * u) - 4 / kPbPi;
        y += (kPbTwoPi * dt) * pb_blamp(u, dt);
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_TRIANGULAR_PULSE) {  // P:234-255
        const double t1 = pb_frac((t + 0.75) + 0.5 * pw);
        double y;
        if (t1 >= pw) {
            y = -pw;
        } else {
            y = 4 * t1;
            y = (y >= 2 * pw ? (4 - y / pw) - pw : y / pw - pw);
        }
        if (pw > 0) {
            const double t2 = pb_frac((t1 + 1) - 0.5 * pw), t3 = pb_frac((t1 + 1) - pw);
            y += ((2 * dt) / pw) * ((pb_blamp(t1, dt) - 2 * pb_blamp(t2, dt)) + pb_blamp(t3, dt));
        }
        return kPbAmp * y;
    } else if constexpr (WF == MXG_PBLEP_TRAPEZOID_FIXED) {  // P:257-285
        double y = pb_fold4(t);
        y = fmax(-1.0, fmin(1.0, 2 * y));
        double t1 = pb_frac(t + 0.125), t2 = pb_frac(t1 + 0.5);
        y += (4 * dt) * (pb_blamp(t1, dt) - pb_blamp(t2, dt));
        t1 = pb_frac(t + 0.375);
        t2 = pb_frac(t1 + 0.5);
        y += (4 * dt) * (pb_blamp(t1, dt) - pb_blamp(t2, dt));
        return kPbAmp * y;
    } else {  // TRAPEZOID_VARIABLE, P:287-318
        static_assert(WF == MXG_PBLEP_TRAPEZOID_VARIABLE, "a waveform of MXG_PBLEP_*");
        const double w = fmin(0.9999, pw);
        const double scale = 1 / (1 - w);
        double y = pb_fold4(t);
        y = fmax(-1.0, fmin(1.0, scale * y));
        double t1 = pb_frac((t + 0.25) - 0.25 * w), t2 = pb_frac(t1 + 0.5);
        y += ((scale * 2) * dt) * (pb_blamp(t1, dt) - pb_blamp(t2, dt));
        t1 = pb_frac((t + 0.25) + 0.25 * w);
        t2 = pb_frac(t1 + 0.5);
        y += ((scale * 2) * dt) * (pb_blamp(t1, dt) - pb_blamp(t2, dt));
        return kPbAmp * y;
    }
}

// maxiPolyBLEP::play(freq): the sample of the phase t, then t advanced (P:114-160)
template <int WF, class SC>
MXG_HD double pb_play(double &t, double freq, double sr, double pw, const SC &sc) {
    const double dt = freq / sr;
    double y;
    if (dt * sr >= sr / 4) y = pb_sin(t, sc);
    else y = pb_wave<WF>(t, dt, pw, sc);
    t += dt;
    t = pb_frac(t);
    return y;
}

// PolyBLEP::sync (P:101-108): a negative phase wraps with t += 1 - (int64)t
MXG_HD double pb_sync(double phase) { return phase >= 0 ? phase - trunc(phase) : phase + (1 - trunc(phase)); }

// a runtime waveform -> pb_play<WF> (host callers; the kernel is instantiated per waveform)
template <class F>
inline bool pb_dispatch(int wf, F &&f) {
    switch (wf) {
#define MXG_PB_CASE(n) case n: f(std::integral_constant<int, n>{}); return true;
        MXG_PB_CASE(0) MXG_PB_CASE(1) MXG_PB_CASE(2) MXG_PB_CASE(3) MXG_PB_CASE(4) MXG_PB_CASE(5) MXG_PB_CASE(6)
        MXG_PB_CASE(7) MXG_PB_CASE(8) MXG_PB_CASE(9) MXG_PB_CASE(10) MXG_PB_CASE(11) MXG_PB_CASE(12) MXG_PB_CASE(13)
#undef MXG_PB_CASE
        default: return false;
    }
}

}  // namespace
}  // namespace mxg
