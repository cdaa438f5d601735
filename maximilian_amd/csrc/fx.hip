// fx.hip -- maxiFlanger and maxiChorus voice banks on gfx950 (K11).
//
// Path (reference src/maximilian.h, cited as H:line): maxiFlanger::flange H:1166-1172, maxiChorus::chorus
// H:1202-1212, over maxiDelayline::dl (C:420-429), maxiOsc::triangle / noise and maxiFilter::lores.  The
// per-sample arithmetic is mxg_fx.h; every step is + - * / or a compare, the lores coefficients come from the
// host libm => bit-exact.
//
// Both effects are a delay line whose tap length changes every sample.  The LFO, the sizes and so the ring's
// slot sequence p(n) do not depend on the audio, so a workgroup of 4 wavefronts owns FX_VB voices and walks the
// block in time tiles of FX_T = 64 samples:
//   1. one lane per voice runs the LFO recurrence over the tile and leaves p(n) in LDS, with the tile's class
//      (mxg_fx.h: touched set = at most two runs, conflict-free iff every slot is touched once);
//   2. meanwhile the other lanes have requested the [N][V] input tile (rows of FX_VB voices), which goes
//      through LDS to be transposed;
//   3. the ring pass: a wavefront takes one voice at a time with one lane per SAMPLE.  A conflict-free tile is
//      64 independent read-modify-writes of one or two contiguous runs of the voice-major ring
//      (mem[v*cap + slot]): coalesced.  The reads of all the wavefront's voices are requested before any of
//      their writes.  A conflicted tile (a size shorter than the tile) stages its <= 2T touched slots in LDS,
//      one lane walks the 64 steps there in order, and the slots go back;
//   4. the output tile leaves through LDS as [N][V] rows.
// A ring cell written in tile t and read in tile t+1 is ordered by the __syncthreads() between the tiles
// (workgroup-scope release / acquire; a voice's ring is only ever touched by its own workgroup).
// Algorithmic traffic: flanger 32 B per sample (in, out, ring read + write); chorus 52 B (two rings + a draw).
#include "mxg_common.h"
#include "mxg_fx.h"

namespace mxg {
namespace {

#ifndef MXG_FX_PROBE
#define MXG_FX_PROBE 0  // 0 = the product; 1 / 2: A/B builds that drop the LFO walk's arithmetic / the ring pass (timing only)
#endif

constexpr int FX_T = 64;                   // samples per tile = lanes of a wavefront
constexpr int FX_VB = 32;                  // voices per workgroup
constexpr int FX_WAVES = 4;                // wavefronts per workgroup
constexpr int FX_VPW = FX_VB / FX_WAVES;   // voices per wavefront in the ring pass
constexpr int FX_QB = 4;                   // ... whose ring reads are in flight together
constexpr int FX_ROWS = 256 / FX_VB;       // tile rows per pass of the whole workgroup

struct FxArgs {
    size_t V, N;
    const double *in;
    const uint32_t *delay;
    const double *feedback, *speed, *depth;  // speed: flanger only
    int ps;                                  // MXG_FX_PS_* bits: that parameter is [N][V]
    const int32_t *rnd;                      // chorus: the draws [N][V]
    const double *coef;                      // chorus: (c, r) [2][V] or [N][2][V]
    int coef_ps;
    double *mem;                             // [R][V][cap]
    int cap;
    int32_t *phase;                          // [R][V]
    double *lfo;                             // flanger: triangle phase [V]; chorus: lores x, y [2][V]
    uint32_t *ovf;                           // [V] or null
    double *out;
    double sr;
};

// a wavefront's LDS writes visible to its other lanes (the compiler keeps the order; the LDS unit does too)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a workgroup barrier that orders LDS only (global loads in flight stay in flight)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <bool CHORUS>
__global__ void __launch_bounds__(256) fx_kernel(FxArgs A) {
    constexpr int R = CHORUS ? 2 : 1;  // rings per voice
    constexpr int T = FX_T;
    __shared__ double io[T][FX_VB + 1];     // input tile, then output tile (padded: the ring pass reads columns)
    __shared__ int sl[R][T][FX_VB + 1];     // p(n) per ring
    __shared__ int info[R][4][FX_VB];       // a0, k, m, conflict
    __shared__ double stg[FX_WAVES][2 * T]; // a conflicted tile's touched slots
    __shared__ double ob[FX_WAVES][T];      // ... and what its walk read
    __shared__ int rsh[CHORUS ? T : 1][FX_VB];  // chorus: the tile's draws

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t V = A.V, N = A.N;
    const size_t v0 = (size_t)blockIdx.x * FX_VB;
    const int cap = A.cap, ps = A.ps;

    // ---- the LFO lanes' state (tid < FX_VB) ----
    const bool p1 = tid < FX_VB && v0 + tid < V;
    const size_t pv = v0 + (p1 ? tid : 0);
    int ph[R];
    double la = 0.0, lb = 0.0, inc = 0.0, cc = 0.0, rr = 0.0, dep = 0.0;
    uint32_t dly = 0, ovf = 0;
    if (p1) {
#pragma unroll
        for (int r = 0; r < R; r++) ph[r] = A.phase[(size_t)r * V + pv];
        la = A.lfo[pv];
        if constexpr (CHORUS) {
            lb = A.lfo[V + pv];
            if (!A.coef_ps) {
                cc = A.coef[pv];
                rr = A.coef[V + pv];
            }
        } else {
            if (!(ps & MXG_FX_PS_SPEED)) inc = fx_tri_inc(A.sr, A.speed[pv]);
        }
        if (!(ps & MXG_FX_PS_DELAY)) dly = A.delay[pv];
        if (!(ps & MXG_FX_PS_DEPTH)) dep = A.depth[pv];
    }

    const int col = tid % FX_VB, row0 = tid / FX_VB;
    const bool colv = v0 + col < V;
    for (size_t n0 = 0; n0 < N; n0 += T) {
        const int nt = (int)((N - n0) < (size_t)T ? (N - n0) : (size_t)T);
        // 2. the input tile is requested first ...
        double xr[T / FX_ROWS];
#pragma unroll
        for (int j = 0; j < T / FX_ROWS; j++) {
            const int row = row0 + j * FX_ROWS;
            xr[j] = (row < nt && colv) ? A.in[(n0 + row) * V + v0 + col] : 0.0;
        }
        // the chorus's draws of the tile are staged in LDS first: a global load inside the serial walk would put a memory latency
        // on every one of its 64 steps (measured: the walk was 0.7 of the chorus's time)
        if constexpr (CHORUS) {
            int rv[T / FX_ROWS];
#pragma unroll
            for (int j = 0; j < T / FX_ROWS; j++) {
                const int row = row0 + j * FX_ROWS;
                rv[j] = (row < nt && colv) ? A.rnd[(n0 + row) * V + v0 + col] : 0;
            }
#pragma unroll
            for (int j = 0; j < T / FX_ROWS; j++) rsh[row0 + j * FX_ROWS][col] = rv[j];
            lds_barrier();
        }
        // 1. ... while the LFO lanes walk the tile
        if (p1) {
            FxTile tl[R];
#pragma unroll
            for (int r = 0; r < R; r++) fx_tile_begin(tl[r]);
            for (int i = 0; i < nt; i++) {
#if MXG_FX_PROBE == 1  // measurement only (an A/B build, tools/build_ab.sh, timed by tools/bench_fx.py): the slot walk without the LFO, the sizes or their loads
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int s = fx_ring_slot(ph[r], cap);
                    fx_tile_add(tl[r], i, s);
                    sl[r][i][tid] = s;
                }
                continue;
#endif
                const size_t e = (n0 + i) * V + pv;
                const uint32_t d = (ps & MXG_FX_PS_DELAY) ? A.delay[e] : dly;
                const double dp = (ps & MXG_FX_PS_DEPTH) ? A.depth[e] : dep;
                if constexpr (!CHORUS) {
                    const double ic = (ps & MXG_FX_PS_SPEED) ? fx_tri_inc(A.sr, A.speed[e]) : inc;
                    const double lfo = fx_triangle(la, ic);
                    const int s = fx_ring_slot(ph[0], fx_ring_size(fx_flanger_size(d, lfo, dp), cap, ovf));
                    fx_tile_add(tl[0], i, s);
                    sl[0][i][tid] = s;
                } else {
                    double c = cc, r = rr;
                    if (A.coef_ps) {
                        const double *cp = A.coef + (n0 + i) * 2 * V + pv;
                        c = cp[0];
                        r = cp[V];
                    }
                    const double lfo = fx_lores(la, lb, fx_noise(rsh[i][tid]), c, r) * 2.0;
                    const int s1 = fx_ring_slot(ph[0], fx_ring_size(fx_flanger_size(d, lfo, dp), cap, ovf));
                    const int s2 = fx_ring_slot(ph[R - 1], fx_ring_size(fx_chorus_size2(d, lfo, dp), cap, ovf));
                    fx_tile_add(tl[0], i, s1);
                    fx_tile_add(tl[R - 1], i, s2);
                    sl[0][i][tid] = s1;
                    sl[R - 1][i][tid] = s2;
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                info[r][0][tid] = tl[r].a0;
                info[r][1][tid] = tl[r].k;
                info[r][2][tid] = tl[r].m;
                info[r][3][tid] = fx_tile_conflict(tl[r]) ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < T / FX_ROWS; j++) io[row0 + j * FX_ROWS][col] = xr[j];
        __syncthreads();

        // 3. the ring pass: this wavefront's voices, one lane per sample
#if MXG_FX_PROBE == 2  // measurement only: no ring pass (the input tile goes straight out)
        const bool act = false;
#else
        const bool act = lane < nt;
#endif
#pragma unroll 1
        for (int qb = 0; qb < FX_VPW; qb += FX_QB) {
        double cur[FX_QB][R];
#pragma unroll
        for (int q = 0; q < FX_QB; q++) {  // every conflict-free read of the batch requested first
            const int l = wave * FX_VPW + qb + q;
#pragma unroll
            for (int r = 0; r < R; r++) {
                cur[q][r] = 0.0;
                if (v0 + l < V && act && !info[r][3][l])
                    cur[q][r] = A.mem[((size_t)r * V + v0 + l) * cap + sl[r][lane][l]];
            }
        }
#pragma unroll
        for (int q = 0; q < FX_QB; q++) {
            const int l = wave * FX_VPW + qb + q;
            const size_t v = v0 + l;
            if (v >= V) break;
            const double x = act ? io[lane][l] : 0.0;
            double o[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                double *m = A.mem + ((size_t)r * V + v) * cap;
                const double fmul = r == 0 ? 1.0 : 0.99;  // dl2 runs at feedback*0.99 (H:1208)
                if (!info[r][3][l]) {
                    if (act) {
                        double fb = (ps & MXG_FX_PS_FEEDBACK) ? A.feedback[(n0 + lane) * V + v] : A.feedback[v];
                        if (r) fb = fb * fmul;
                        o[r] = cur[q][r];
                        m[sl[r][lane][l]] = fx_ring_update(cur[q][r], x, fb);
                    }
                } else {
                    FxTile t;
                    t.a0 = info[r][0][l];
                    t.k = info[r][1][l];
                    t.m = info[r][2][l];
                    const int sa = fx_stage_slot_a(t, lane), sb = fx_stage_slot_b(t, lane);
                    if (sa >= 0) stg[wave][lane] = m[sa];
                    if (sb >= 0) stg[wave][T + lane] = m[sb];
                    wave_sync();
                    if (lane == 0) {
                        for (int i = 0; i < nt; i++) {
                            double fb = (ps & MXG_FX_PS_FEEDBACK) ? A.feedback[(n0 + i) * V + v] : A.feedback[v];
                            if (r) fb = fb * fmul;
                            const int k = fx_stage_index(t, sl[r][i][l], T);
                            const double c = stg[wave][k];
                            ob[wave][i] = c;
                            stg[wave][k] = fx_ring_update(c, io[i][l], fb);
                        }
                    }
                    wave_sync();
                    if (act) o[r] = ob[wave][lane];
                    if (sa >= 0) m[sa] = stg[wave][lane];
                    if (sb >= 0) m[sb] = stg[wave][T + lane];
                    wave_sync();  // the staging buffer is free again
                }
            }
            if (act) {
                if constexpr (CHORUS) io[lane][l] = fx_chorus_out(o[0], o[R - 1], x);
                else io[lane][l] = fx_flanger_out(o[0], x);
            }
        }
        }
        __syncthreads();

        // 4. the output tile
#pragma unroll
        for (int j = 0; j < T / FX_ROWS; j++) {
            const int row = row0 + j * FX_ROWS;
            if (row < nt && colv) A.out[(n0 + row) * V + v0 + col] = io[row][col];
        }
        __syncthreads();
    }

    if (p1) {
#pragma unroll
        for (int r = 0; r < R; r++) A.phase[(size_t)r * V + pv] = ph[r];
        A.lfo[pv] = la;
        if constexpr (CHORUS) A.lfo[V + pv] = lb;
        if (A.ovf) A.ovf[pv] += ovf;
    }
}

int fx_launch(bool chorus, FxArgs &A, hipStream_t st) {
    A.sr = (double)settings().sampleRate;
    const dim3 grid((unsigned)((A.V + FX_VB - 1) / FX_VB));
    if (chorus) {
        KernelTimer kt("fx_chorus_kernel", st);
        hipLaunchKernelGGL(fx_kernel<true>, grid, dim3(256), 0, st, A);
        return check_hip(hipGetLastError(), "fx_chorus_kernel launch");
    }
    KernelTimer kt("fx_flanger_kernel", st);
    hipLaunchKernelGGL(fx_kernel<false>, grid, dim3(256), 0, st, A);
    return check_hip(hipGetLastError(), "fx_flanger_kernel launch");
}
}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_flanger_render(size_t V, size_t N, const double *d_in, const uint32_t *d_delay, const double *d_feedback,
                       const double *d_speed, const double *d_depth, int ps_flags, double *d_mem, size_t cap,
                       int32_t *d_phase, double *d_lfo_phase, uint32_t *d_overflow, double *d_out, void *stream) {
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(d_in && d_delay && d_feedback && d_speed && d_depth && d_mem && d_phase && d_lfo_phase && d_out,
                "null device pointer");
    MXG_REQUIRE(cap > 0 && cap <= 0x7fffffff, "cap must be in 1 .. 2^31-1");
    MXG_REQUIRE((ps_flags & ~MXG_FX_PS_ALL) == 0, "unknown ps_flags bit");
    if (V == 0 || N == 0) return MXG_OK;
    FxArgs A = {V, N, d_in, d_delay, d_feedback, d_speed, d_depth, ps_flags, nullptr, nullptr, 0,
                d_mem, (int)cap, d_phase, d_lfo_phase, d_overflow, d_out, 0.0};
    return fx_launch(false, A, resolve_stream(stream));
}

int mxg_chorus_render(size_t V, size_t N, const double *d_in, const uint32_t *d_delay, const double *d_feedback,
                      const double *d_depth, int ps_flags, const int32_t *d_rand, const double *d_coef, int coef_ps,
                      double *d_mem, size_t cap, int32_t *d_phase, double *d_lp, uint32_t *d_overflow, double *d_out,
                      void *stream) {
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(d_in && d_delay && d_feedback && d_depth && d_rand && d_coef && d_mem && d_phase && d_lp && d_out,
                "null device pointer");
    MXG_REQUIRE(cap > 0 && cap <= 0x7fffffff, "cap must be in 1 .. 2^31-1");
    MXG_REQUIRE((ps_flags & ~(MXG_FX_PS_DELAY | MXG_FX_PS_FEEDBACK | MXG_FX_PS_DEPTH)) == 0,
                "unknown ps_flags bit (the chorus's speed is its coefficients: coef_ps)");
    MXG_REQUIRE(coef_ps == 0 || coef_ps == 1, "coef_ps must be 0 ([2][V]) or 1 ([N][2][V])");
    if (V == 0 || N == 0) return MXG_OK;
    FxArgs A = {V, N, d_in, d_delay, d_feedback, nullptr, d_depth, ps_flags, d_rand, d_coef, coef_ps,
                d_mem, (int)cap, d_phase, d_lp, d_overflow, d_out, 0.0};
    return fx_launch(true, A, resolve_stream(stream));
}

}  // extern "C"
