// mxg_drums.h -- the reference's three drum voices (src/libs/maxiSynths.cpp:11-259) and its metronome (src/libs/maxiClock.cpp) as
// plain per-sample arithmetic: one step function per drum plus clock_tick.  No device state: the same text compiles for the host
// (mxg_drum_host / mxg_clock_host, tests/host_drums.cpp) and for the kernels of drums.hip (K21).  Nothing is restated here that the
// library already has: the envelope is env_adsr (mxg_env.h), the noise and the lores fx_noise / fx_lores (mxg_fx.h), the distortion
// shp_fastatandist (mxg_shaper.h), the triangle, sinebuf and phasor osc_pre / osc_tick (mxg_osc.h, the phasor through seq_clock_tick),
// the kick's sine sincos_tab on the rounded product (mxg_sincos.h: the body of sin_2pi_phase, which is a device-only wrapper) and the hats' filter svf_step (mxg_svf.h).  The reference's expression trees, never
// contracted.
//
// All three play() calls share one frame (S = maxiSynths.cpp):
//     envOut = envelope.adsr(1., envelope.trigger);  if (inverse) envOut = fabs(1 - envOut);           S:25-31
//     output = <the voice>;  envelope.trigger goes back to 0 if it was 1                                S:33-37
//     if (useDistortion) output = distort.fastAtanDist(output, distortion);                             S:39-42
//     if (useFilter) output = <the filter>;                                                             S:44-48
//     if (useLimiter) return output*gain clipped to exactly +-1, else return output*gain                S:50-72
//   kick   kick.sinewave(pitch*envOut)*envOut, lores.   Before the first trigger envOut is 0: sinewave(0) steps the phase by
//          1/(sr/0) = 1/inf = 0 -- no branch, but the division is IEEE.  The one inexact operation is the sine (<= 1 ULP).
//   snare  (tone.triangle(pitch*(0.1+(envOut*0.85))) + noise.noise())*envOut, lores
//   hats   (tone.sinebuf(pitch) + noise.noise())*envOut, maxiSVF::play(output, 0., 0., 1., 0.)
// trigger() only sets envelope.trigger = 1 and play() clears it, so the trigger is an INPUT of the step (`trig`: was trigger() called
// before this play()), not a state.  noise() takes one rand() draw per play(): the caller supplies it (`rnd`), as for mxg_osc_noise.
// Everything but the kick's sine is compares, + - * /, floor, table reads and float arithmetic on the draw: bit-exact.
//
// maxiClock::ticker(): tick = false; currentCount = floor(timer.phasor(bps)); if (lastCount != currentCount) { tick = true;
// playHead++; } -- ticker never writes lastCount, so with lastCount = 0 a tick is the one sample per wrap on which the phasor
// returns a phase >= 1.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "mxg_hd.h"
#include "mxg_osc.h"
#include "mxg_env.h"
#include "mxg_fx.h"
#include "mxg_seq.h"
#include "mxg_shaper.h"
#include "mxg_sincos.h"
#include "mxg_svf.h"

// include/maxigpu.h, where it is included, comes first and has these
#ifndef MXG_DRUM_KINDS
#define MXG_DRUM_KICK 0
#define MXG_DRUM_SNARE 1
#define MXG_DRUM_HATS 2
#define MXG_DRUM_KINDS 3
#define MXG_DRUM_INVERSE 1
#define MXG_DRUM_DISTORTION 2
#define MXG_DRUM_FILTER 4
#define MXG_DRUM_LIMITER 8
#endif

namespace mxg {
namespace {

struct DrumPar {
    double pitch, shape, gain;
    double c[5];  // kick / snare: lores' (c, r); hats: g1, g2, g3, g4, k
    OscPre q;     // hats: sinebuf's increment, constant per voice
    double sr;    // (double)maxiSettings::sampleRate
    int flags;    // MXG_DRUM_*: constant per call
};

struct DrumState {
    double phase;       // kick.phase / tone.phase
    Env env;            // envelope
    double f0, f1, f2;  // filter.x, filter.y, unused | filter.v0z, v1, v2
};

template <int KIND>
MXG_HD void drum_par_init(DrumPar &p) {
    if constexpr (KIND == MXG_DRUM_HATS) p.q = osc_pre<MXG_OSC_SINEBUF>(p.pitch, p.sr, 0.0, 0.0);
}

// One play().  tab: the kick's sin / cos table (MXG_SINTAB, mxg_sincos.h), the hats' sineBuffer with its guard entry (maxi_tables.h);
// unused by the snare.  rnd: this call's rand() draw (snare, hats).
template <int KIND>
MXG_HD double drum_step(DrumState &s, const DrumPar &p, bool trig, int32_t rnd, const double *tab, const SinTabK k) {
    double envOut = env_adsr(s.env, 1., trig ? 1 : 0);
    if (p.flags & MXG_DRUM_INVERSE) envOut = fabs(1 - envOut);
    double output, hold;
    if constexpr (KIND == MXG_DRUM_KICK) {  // maxiOsc::sinewave C:228-235
        const double f = p.pitch * envOut;
        const double r = sincos_tab<false>(s.phase * (MXG_TWOPI), tab, k);
        if (s.phase >= 1.0) s.phase -= 1.0;
        s.phase += (1. / (p.sr / (f)));
        output = r * envOut;
    } else if constexpr (KIND == MXG_DRUM_SNARE) {
        const OscPre q = osc_pre<MXG_OSC_TRIANGLE>(p.pitch * (0.1 + (envOut * 0.85)), p.sr, 0.0, 0.0);
        output = (osc_tick<MXG_OSC_TRIANGLE>(s.phase, hold, q, nullptr, nullptr) + fx_noise(rnd)) * envOut;
    } else {
        output = (osc_tick<MXG_OSC_SINEBUF>(s.phase, hold, p.q, tab, nullptr) + fx_noise(rnd)) * envOut;
    }
    if (p.flags & MXG_DRUM_DISTORTION) output = shp_fastatandist(output, p.shape);
    if (p.flags & MXG_DRUM_FILTER) {
        if constexpr (KIND == MXG_DRUM_HATS) {
            const double c[9] = {p.c[0], p.c[1], p.c[2], p.c[3], p.c[4], 0., 0., 1., 0.};
            output = svf_step(s.f0, s.f1, s.f2, output, c);
        } else {
            output = fx_lores(s.f0, s.f1, output, p.c[0], p.c[1]);
        }
    }
    const double g = output * p.gain;
    if (p.flags & MXG_DRUM_LIMITER) return g > 1 ? 1. : (g < -1 ? -1. : g);
    return g;
}

// One ticker().  q: osc_pre<MXG_OSC_PHASOR>(bps); returns tick, writes currentCount.  The conversion of floor()'s double to the
// int member is x86-64's (fx_cvt_i32).
MXG_HD bool clock_tick(double &clk, const OscPre &q, int32_t lastCount, int32_t &currentCount, long long &playHead) {
    currentCount = fx_cvt_i32(floor(seq_clock_tick(clk, q)));
    const bool tick = lastCount != currentCount;
    playHead += tick ? 1 : 0;
    return tick;
}

// ---- a launch's arguments, and a voice's way in and out of them (arrays on the device or on the host) --------------------------------
struct DrumArgs {
    size_t V, N;
    size_t tstride;  // rows of the trigger block: V apart (one per voice) or 1 (shared)
    const double *pitch, *par;
    const int64_t *holdtime;
    const double *shape, *coef, *gain;
    double sr;
    int flags;
    double *phase, *dst;
    int64_t *ist;
    double *fst;
    int px_store;
};

// the parameters and the state of voice v (arrays on the device or on the host)
template <int KIND>
MXG_HD void drum_load(const DrumArgs &A, size_t v, DrumPar &p, DrumState &s) {
    const size_t V = A.V;
    p.pitch = A.pitch[v];
    p.shape = A.shape ? A.shape[v] : 0.0;
    p.gain = A.gain ? A.gain[v] : 1.0;
    constexpr int NC = KIND == MXG_DRUM_HATS ? 5 : 2;
#pragma unroll
    for (int r = 0; r < 5; r++) p.c[r] = (r < NC && A.coef) ? A.coef[(size_t)r * V + v] : 0.0;
    p.sr = A.sr;
    p.flags = A.flags;
    drum_par_init<KIND>(p);
    s.phase = A.phase[v];
    env_load(s.env, V, v, A.par, A.holdtime, A.dst, A.ist);
    s.f0 = A.fst[v];
    s.f1 = A.fst[V + v];
    s.f2 = A.fst[2 * V + v];
}
MXG_HD void drum_store(const DrumArgs &A, size_t v, const DrumState &s) {
    const size_t V = A.V;
    A.phase[v] = s.phase;
    env_store(s.env, V, v, A.dst, A.ist);
    A.fst[v] = s.f0;
    A.fst[V + v] = s.f1;
    A.fst[2 * V + v] = s.f2;
}

// the host form of a launch: voice after voice, sample after sample (mxg_drum_host, tests/host_drums.cpp)
template <int KIND>
void drum_host_run(const DrumArgs &A, const double *trig, int tpv, const int32_t *rnd, double *out, const double *sintab, const double *sinebuf) {
    const double *tab = KIND == MXG_DRUM_KICK ? sintab : sinebuf;
    for (size_t v = 0; v < A.V; v++) {
        DrumPar p;
        DrumState s;
        drum_load<KIND>(A, v, p, s);
        for (size_t n = 0; n < A.N; n++) {
            const bool t = trig && trig[tpv ? n * A.V + v : n] != 0.0;
            out[n * A.V + v] = drum_step<KIND>(s, p, t, rnd ? rnd[n * A.V + v] : 0, tab, {1.0 / 120, 1.0 / 24});
        }
        drum_store(A, v, s);
    }
}

template <typename F>
bool drum_dispatch(int kind, F &&f) {
    switch (kind) {
        case MXG_DRUM_KICK: f(std::integral_constant<int, MXG_DRUM_KICK>{}); return true;
        case MXG_DRUM_SNARE: f(std::integral_constant<int, MXG_DRUM_SNARE>{}); return true;
        case MXG_DRUM_HATS: f(std::integral_constant<int, MXG_DRUM_HATS>{}); return true;
    }
    return false;
}

}  // namespace
}  // namespace mxg
