// drums.hip -- maxiKick / maxiSnare / maxiHats banks and the maxiClock bank on gfx950 (K21): the reference's three drum voices
// (src/libs/maxiSynths.cpp:11-259) fused into one kernel per voice kind, and its metronome (src/libs/maxiClock.cpp).  The per-sample
// arithmetic is mxg_drums.h, which also compiles for the host (mxg_drum_host / mxg_clock_host below, tests/host_drums.cpp).
//
// drum_kernel has the streaming shape of mxg_stream.h: one lane = one voice, chunks of 8 samples, surplus lanes shadow a voice (the
// last pair with pair rows) and store no state, whole chunks leave through emit_chunk, a ragged last chunk by 8-byte stores.  The
// [N][V] inputs -- the trigger block (doubles) and, for snare and hats, the int32 rand() draws -- are requested a chunk ahead with the
// clamped prefetch; everything loaded in the prologue is consumed before the loop.  The drum kind is a template argument.  The four
// switches (inverse, useDistortion, useFilter, useLimiter) are constant per call and reach the kernel as ONE wave-uniform flag word:
// four scalar branches per sample next to the voice's FP64 arithmetic, against 16 instantiations of each of the 12 kernels as
// template arguments.
// HBM per sample: 8 B out; + 8 B with a per-voice trigger block; + 4 B for the draw of snare and hats.
// LDS: kick the 16 KB sin / cos table of mxg_sincos.h (as polyblep.hip), hats the 515-entry sineBuffer (as osc.hip), snare none.
// No scratch.
#include "mxg_drums.h"

#include <math.h>

#include "maxi_tables.h"
#include "mxg_common.h"
#include "mxg_stream.h"

namespace mxg {
namespace {

__device__ const double MXG_DR_SINTAB_D[MXG_SINTAB_LEN] = {MXG_SINTAB_VALUES};
const double kDrSinTabHost[MXG_SINTAB_LEN] = {MXG_SINTAB_VALUES};
__device__ const double MXG_DR_SINEBUF_D[MAXI_SINE_TAB_LEN] = MAXI_SINE_TAB_INIT;
const double kDrSineBufHost[MAXI_SINE_TAB_LEN] = MAXI_SINE_TAB_INIT;

template <int KIND>
constexpr int drum_tab_len() {
    return KIND == MXG_DRUM_KICK ? MXG_SINTAB_LEN : (KIND == MXG_DRUM_HATS ? MAXI_SINE_TAB_LEN : 1);
}

// TRIG: a trigger block; without one no voice is ever triggered.  trig / rnd / out are separate __restrict__ parameters.
template <int KIND, bool TRIG, bool PX>
__global__ void __launch_bounds__(256) drum_kernel(DrumArgs A, const double *__restrict__ trig, const int32_t *__restrict__ rnd,
                                                   double *__restrict__ out_ptr) {
    constexpr bool RND = KIND != MXG_DRUM_KICK;
    const double *s_tab = nullptr;  // (the snare reads no table)
    if constexpr (KIND != MXG_DRUM_SNARE) {
        __shared__ double tab[drum_tab_len<KIND>()];
        const double *src = KIND == MXG_DRUM_KICK ? MXG_DR_SINTAB_D : MXG_DR_SINEBUF_D;
        for (int i = threadIdx.x; i < drum_tab_len<KIND>(); i += blockDim.x) tab[i] = src[i];
        __syncthreads();
        s_tab = tab;
    }
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const bool live = gid < V;
    const size_t v = bank_voice<PX>(gid, V);
    DrumPar p;
    DrumState s;
    drum_load<KIND>(A, v, p, s);
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(p.pitch), "+v"(p.shape), "+v"(p.gain), "+v"(p.c[0]), "+v"(p.c[1]), "+v"(p.c[2]), "+v"(p.c[3]), "+v"(p.c[4]));
    asm volatile("" : "+v"(s.phase), "+v"(s.f0), "+v"(s.f1), "+v"(s.f2), "+v"(s.env.attack), "+v"(s.env.decay), "+v"(s.env.sustain),
                 "+v"(s.env.release), "+v"(s.env.amplitude), "+v"(s.env.output));
    asm volatile("" : "+v"(s.env.holdtime), "+v"(s.env.holdcount), "+v"(s.env.attackphase), "+v"(s.env.decayphase),
                 "+v"(s.env.sustainphase), "+v"(s.env.holdphase), "+v"(s.env.releasephase));
    const SinTabK k = sintab_k();
    constexpr int U = 8;
    const size_t ts = A.tstride;
    const double *__restrict__ tp = TRIG ? trig + (ts == 1 ? 0 : v) : nullptr;
    const int32_t *__restrict__ rp = RND ? rnd + v : nullptr;
    double *op = out_ptr + v;
    double tn[U];
    int32_t rn[U];
    if constexpr (TRIG) rows_first(tn, tp, ts, N);
    if constexpr (RND) rows_first(rn, rp, V, N);
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double tc[U];
        int32_t rc[U];
        if constexpr (TRIG) rows_next(tc, tn, tp, ts, N, n0);
        if constexpr (RND) rows_next(rc, rn, rp, V, N, n0);
        const int cnt = n0 + U <= N ? U : (int)(N - n0);  // (wave-uniform, mxg_stream.h)
        double y[U];
#pragma unroll
        for (int i = 0; i < U; i++) {
            y[i] = drum_step<KIND>(s, p, TRIG ? tc[i] != 0.0 : false, RND ? rc[i] : 0, s_tab, k);
            if (i + 1 == cnt) break;
        }
        emit_rows<PX>(op, V, y, cnt, A.px_store);
    }
    if (!live) return;  // a shadow lane owns no state
    drum_store(A, v, s);
}

// maxiClock::ticker() N times per voice: the tick block [N][V] (1.0 / 0.0), the phasor's phase and playHead carried, currentCount out
__global__ void __launch_bounds__(256) clock_kernel(size_t V, size_t N, const double *__restrict__ bps, double sr, double *__restrict__ clk,
                                                    const int32_t *__restrict__ lastcount, int64_t *__restrict__ playhead,
                                                    int32_t *__restrict__ count, double *__restrict__ tick) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const OscPre q = osc_pre<MXG_OSC_PHASOR>(bps[v], sr, 0.0, 0.0);
    double c = clk[v];
    const int32_t last = lastcount ? lastcount[v] : 0;
    long long ph = playhead[v];
    int32_t cur = 0;
    double *tp = tick + v;
    for (size_t n = 0; n < N; n++) {
        *tp = clock_tick(c, q, last, cur, ph) ? 1.0 : 0.0;
        tp += V;
    }
    clk[v] = c;
    playhead[v] = ph;
    count[v] = cur;
}

bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && x < y + bbytes && y < x + abytes;
}

}  // namespace
}  // namespace mxg

using namespace mxg;

// the argument checks of mxg_drum_render and mxg_drum_host: the same refusals, with the same messages, on device and host arrays
#define MXG_DRUM_CHECKS()                                                                                                           \
    MXG_REQUIRE(V > 0 && N > 0, "V and N must be at least 1");                                                                      \
    MXG_REQUIRE(kind >= 0 && kind < MXG_DRUM_KINDS, "kind is not one of MXG_DRUM_KICK, MXG_DRUM_SNARE, MXG_DRUM_HATS");             \
    MXG_REQUIRE((flags & ~15) == 0, "flags has bits outside MXG_DRUM_INVERSE | DISTORTION | FILTER | LIMITER");                     \
    MXG_REQUIRE(kind == MXG_DRUM_KICK || rnd, "the rand() draws are required for snare and hats");                                  \
    MXG_REQUIRE(kind != MXG_DRUM_KICK || !rnd, "the kick draws no rand(): pass NULL for the draws");                                \
    MXG_REQUIRE(pitch, "the pitch array is null");                                                                                  \
    MXG_REQUIRE(env_par && holdtime, "the envelope parameters (env_par, holdtime) are null");                                       \
    MXG_REQUIRE(!(flags & MXG_DRUM_DISTORTION) || shape, "useDistortion needs the shape array");                                    \
    MXG_REQUIRE(!(flags & MXG_DRUM_FILTER) || coef, "useFilter needs the coefficient array");                                       \
    MXG_REQUIRE(phase && dst && ist && fst, "a state array (phase, dst, ist, fst) is null");                                        \
    MXG_REQUIRE(out, "the output block is null");                                                                                   \
    MXG_REQUIRE(!ranges_overlap(out, N * V * 8, trig, (tpv ? N * V : N) * 8) && !ranges_overlap(out, N * V * 8, rnd, N * V * 4),    \
                "the output block overlaps an input block")

extern "C" {

int mxg_drum_host(int kind, int flags, size_t V, size_t N, const double *trig, int tpv, const int32_t *rnd, const double *pitch,
                  const double *env_par, const int64_t *holdtime, const double *shape, const double *coef, const double *gain,
                  double *phase, double *dst, int64_t *ist, double *fst, double *out) {
    MXG_DRUM_CHECKS();
    const DrumArgs A = {V, N, tpv ? V : 1, pitch, env_par, holdtime, shape, coef, gain, (double)settings().sampleRate, flags,
                        phase, dst, ist, fst, 0};
    drum_dispatch(kind, [&](auto K) { drum_host_run<decltype(K)::value>(A, trig, tpv, rnd, out, kDrSinTabHost, kDrSineBufHost); });
    return MXG_OK;
}

int mxg_drum_render(int kind, int flags, size_t V, size_t N, const double *trig, int tpv, const int32_t *rnd, const double *pitch,
                    const double *env_par, const int64_t *holdtime, const double *shape, const double *coef, const double *gain,
                    double *phase, double *dst, int64_t *ist, double *fst, double *out, void *stream) {
    MXG_DRUM_CHECKS();
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    const int block = voice_block(V, true);
    const DrumArgs A = {V, N, tpv ? V : 1, pitch, env_par, holdtime, shape, coef, gain, (double)settings().sampleRate, flags,
                        phase, dst, ist, fst, rw_store_choice(V, N, out, (trig || rnd) ? RW_READ_WRITE : RW_WRITE_ONLY)};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("drum_kernel", st);
    drum_dispatch(kind, [&](auto K) {
        with_bools([&](auto TRIG, auto PX) {
            hipLaunchKernelGGL((drum_kernel<decltype(K)::value, TRIG.value, PX.value>), voice_grid(V, block), dim3(block), 0, st, A, trig,
                               rnd, out);
        }, trig != nullptr, A.px_store != 0);
    });
    return check_hip(hipGetLastError(), "drum_kernel launch");
}

#define MXG_CLOCK_CHECKS()                                         \
    MXG_REQUIRE(V > 0 && N > 0, "V and N must be at least 1");     \
    MXG_REQUIRE(bps, "the bps array is null");                     \
    MXG_REQUIRE(clk, "the phase array (clk) is null");             \
    MXG_REQUIRE(playhead, "the playhead array is null");           \
    MXG_REQUIRE(count, "the count array is null");                 \
    MXG_REQUIRE(tick, "the tick block is null");                   \
    MXG_REQUIRE(!ranges_overlap(tick, N * V * 8, bps, V * 8) && !ranges_overlap(tick, N * V * 8, clk, V * 8) &&                \
                    !ranges_overlap(tick, N * V * 8, lastcount, V * 4) && !ranges_overlap(tick, N * V * 8, playhead, V * 8) && \
                    !ranges_overlap(tick, N * V * 8, count, V * 4),                                                            \
                "the tick block overlaps another array")

int mxg_clock_host(size_t V, size_t N, const double *bps, double *clk, const int32_t *lastcount, int64_t *playhead, int32_t *count,
                   double *tick) {
    MXG_CLOCK_CHECKS();
    const double sr = (double)settings().sampleRate;
    for (size_t v = 0; v < V; v++) {
        const OscPre q = osc_pre<MXG_OSC_PHASOR>(bps[v], sr, 0.0, 0.0);
        double c = clk[v];
        long long ph = playhead[v];
        int32_t cur = 0;
        for (size_t n = 0; n < N; n++) tick[n * V + v] = clock_tick(c, q, lastcount ? lastcount[v] : 0, cur, ph) ? 1.0 : 0.0;
        clk[v] = c;
        playhead[v] = ph;
        count[v] = cur;
    }
    return MXG_OK;
}

int mxg_clock_render(size_t V, size_t N, const double *bps, double *clk, const int32_t *lastcount, int64_t *playhead, int32_t *count,
                     double *tick, void *stream) {
    MXG_CLOCK_CHECKS();
    if (int s = ensure_init()) return s;
    const int block = voice_block(V, true);
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("clock_kernel", st);
    hipLaunchKernelGGL(clock_kernel, voice_grid(V, block), dim3(block), 0, st, V, N, bps, (double)settings().sampleRate, clk, lastcount,
                       playhead, count, tick);
    return check_hip(hipGetLastError(), "clock_kernel launch");
}

}  // extern "C"
