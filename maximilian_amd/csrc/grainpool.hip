// grainpool.hip -- K27: granular streams over the slots of a sample pool (maxiTimeStretch / maxiPitchShift / maxiStretch objects
// that each had their own setSample), maxiStretch's loop points and playAtPosition, parameters readable at every sample.  The
// arithmetic is mxg_grainpool.h's; this file is the kernel, the argument checks and the C-ABI.
//
// grainpool_walk_kernel: one lane per stream walks the call's T samples with up to 8 live grains in registers in creation order,
// like K8 (grains.hip granular_kernel) -- but the sample pointer, its length, the loop and, under the MXG_GPOOL_PS_* bits, speed /
// rate / position / posMod are the stream's own, read where the reference's play() would be handed them.  The window table is
// staged in LDS (the one table all streams of a plan share); the [T][S] block is written sample-major, so the 64 lanes of a
// wavefront store one 512-byte run per sample; a slot is read by the lanes that were pointed at it (neighbouring grains of streams
// on the same slot share lines, streams on different slots do not).
#include "mxg_common.h"
#include "mxg_grainplan.h"
#include "mxg_grainpool.h"

#include <vector>

namespace mxg {

// grainpool_host.cpp: the same header compiled as plain C++
int grainpool_host_render(int mode, const GpArgs &A);
const char *grainpool_stretch_loop(uint64_t len, double start01, double end01, uint64_t *loopStart, uint64_t *loopEnd);

namespace {

template <int MODE>
__global__ __launch_bounds__(64) void grainpool_walk_kernel(const GpArgs A, int *err, int winInLds) {
    extern __shared__ double s_gpwin[];
    const double *win = A.window;
    if (winInLds) {
        for (int i = threadIdx.x; i < A.sampleDur; i += blockDim.x) s_gpwin[i] = A.window[i];
        __syncthreads();
        win = s_gpwin;
    }
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.S) return;
    const int failed = gp_walk_stream<MODE>(A, s, win);
    if (failed) atomicMax(err, failed);
}

// ---- the tile form (mxg_grainpool.h: gp_tile_sched, gp_tile_sample) -----------------------------------------------------------
// grainpool_sched_kernel: one lane per stream, the scheduler alone -- births, the per-tile counts, the state of the call's end.
// grainpool_tile_kernel: a workgroup renders kGpTileStreams streams x 64 samples.  Each of its four wavefronts takes four streams in
// turn; inside a wavefront the 64 lanes are 64 consecutive samples of ONE stream, so a grain's reads in its slot are neighbours and
// its window reads are a contiguous run of the table in LDS, and the loops over a stream's grains are uniform.  The results cross
// an LDS tile (rows padded to 17 doubles) so that the block leaves as rows of 16 consecutive streams = one 128-byte line each.
constexpr size_t kGpAutoTiles = 128;  // knob 0: calls of at least this many samples take the tile form (tools/bench_grainpool.py)
constexpr int kGpTileStreams = 16, kGpTileThreads = 256, kGpTilePitch = kGpTileStreams + 1;

template <int MODE>
__global__ __launch_bounds__(64) void grainpool_sched_kernel(const GpArgs A, const GpLists L, int *err) {
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.S) return;
    const int failed = gp_tile_sched<MODE>(A, L, s);
    if (failed) atomicMax(err, failed);
}

__global__ __launch_bounds__(kGpTileThreads) void grainpool_tile_kernel(const GpArgs A, const GpLists L, int winPad) {
    extern __shared__ double s_gptile[];  // the window table | the tile [64][17]
    double *win = s_gptile, *tile = s_gptile + winPad;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < A.sampleDur; i += kGpTileThreads) win[i] = A.window[i];
    __syncthreads();
    const size_t s0 = (size_t)blockIdx.x * kGpTileStreams;
    const int n0 = (int)blockIdx.y * kGpTile;
#pragma unroll 1
    for (int q = 0; q < kGpTileStreams / 4; q++) {
        const int sl = wave * (kGpTileStreams / 4) + q;
        const size_t s = s0 + (size_t)sl;
        double v = 0.0;
        if (s < A.S && (size_t)(n0 + lane) < A.T) v = gp_tile_sample(A, L, s, n0, lane, win);
        tile[lane * kGpTilePitch + sl] = v;
    }
    __syncthreads();
    for (int e = tid; e < kGpTile * kGpTileStreams; e += kGpTileThreads) {
        const int row = e / kGpTileStreams, col = e % kGpTileStreams;
        if ((size_t)(n0 + row) < A.T && s0 + (size_t)col < A.S) A.out[(size_t)(n0 + row) * A.S + s0 + (size_t)col] = tile[row * kGpTilePitch + col];
    }
}

// forwards the call's error word to the library's async error word and leaves it at zero for the next call (grains.hip's protocol
// for the per-stream words of SCR_GRAIN_ERR)
__global__ void grainpool_err_publish_kernel(int *err, int *async_word) {
    const int e = err[0];
    if (e && async_word) __hip_atomic_store(async_word, (int)ASYNC_GRAIN_BASE + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    err[0] = 0;
}

int grainpool_check(const char *fn, const mxg_grain_plan *p, int mode, size_t S, size_t T, const double *pool, size_t stride,
                    size_t cap, size_t R, const uint64_t *len, const uint32_t *slot, int overlaps, const double *a, const double *b,
                    int ps_flags, const double *st, const double *gst, const double *out) {
#define GP_REQ(cond, msg) \
    do { if (!(cond)) return fail(MXG_ERR_INVALID, "%s: %s", fn, msg); } while (0)
    GP_REQ(p, "the plan is null");
    GP_REQ(mode >= 0 && mode <= 4, "mode must be 0 (maxiTimeStretch::play), 1 (maxiStretch::play), 2 (maxiTimeStretch::playAtPosition), 3 "
                                   "(maxiPitchShift::play) or 4 (maxiStretch::playAtPosition)");
    GP_REQ(pool, "the pool is null");
    GP_REQ(R != 0, "R is 0");
    GP_REQ(cap != 0 && cap <= ((size_t)1 << 31) - 256, "cap is 0 or larger than 2^31 - 256");
    GP_REQ(R == 1 || stride >= cap, "stride is smaller than cap (with more than one slot)");
    GP_REQ(len, "len is null");
    GP_REQ(slot || S <= R, "slot is null and S is larger than R");
    GP_REQ(overlaps > 0, "overlaps <= 0");
    GP_REQ(a, "a is null");
    GP_REQ((mode != 1 && mode != 4) || b, mode == 1 ? "b (timestretch) is null (mode 1)" : "b (the position) is null (mode 4)");
    GP_REQ((ps_flags & ~(MXG_GPOOL_PS_A | MXG_GPOOL_PS_B | MXG_GPOOL_PS_POSMOD)) == 0, "ps_flags has bits other than MXG_GPOOL_PS_A | _B | _POSMOD");
    GP_REQ(st, "st is null");
    GP_REQ(gst, "gst is null");
    GP_REQ(out, "the output block out is null");
    GP_REQ(T <= ((size_t)1 << 30), "T is larger than 2^30");
#undef GP_REQ
    return MXG_OK;
}

int grainpool_slots_check(const char *fn, size_t S, size_t R, const uint32_t *h_slot) {
    for (size_t s = 0; s < S; s++)
        if (h_slot[s] >= R) return fail(MXG_ERR_INVALID, "%s: slot[%zu] = %u is outside the pool of R = %zu slots", fn, s, h_slot[s], R);
    return MXG_OK;
}

GpArgs grainpool_args(const mxg_grain_plan *p, const double *window, size_t S, size_t T, const double *pool, size_t stride, size_t cap, size_t R,
                      const uint64_t *len, const uint32_t *slot, const uint64_t *loop, int overlaps, const double *a, const double *b,
                      const double *posmod, int ps_flags, const int32_t *rnd, size_t Rn, double *st, double *gst, double *out) {
    GpArgs A;
    A.S = S; A.T = T; A.R = R; A.stride = stride; A.cap = cap; A.Rn = Rn;
    A.pool = pool; A.len = len; A.slot = slot; A.loop = loop; A.window = window;
    A.a = a; A.b = b; A.posMod = posmod; A.ps = ps_flags; A.rnd = rnd;
    A.st = st; A.gst = gst; A.out = out;
    A.sr = (double)settings().sampleRate;
    A.cycleLength = p->grainLength * settings().sampleRate / overlaps;  // L/maxiGrains.h:346 / :518
    A.grainLength = p->grainLength;
    A.sampleDur = (int)p->sampleDur;
    return A;
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_stretch_loop_host(uint64_t len, double start01, double end01, uint64_t *loopStart, uint64_t *loopEnd) {
    MXG_REQUIRE(loopStart && loopEnd, "loopStart or loopEnd is null");
    MXG_REQUIRE(len != 0, "len is 0");
    if (const char *why = grainpool_stretch_loop(len, start01, end01, loopStart, loopEnd)) return fail(MXG_ERR_INVALID, "%s: %s", __func__, why);
    return MXG_OK;
}

int mxg_granular_pool_render(const mxg_grain_plan *p, int mode, size_t S, size_t T, const double *d_pool, size_t stride, size_t cap, size_t R,
                             const uint64_t *d_len, const uint32_t *d_slot, const uint64_t *d_loop, int overlaps, const double *d_a,
                             const double *d_b, const double *d_posmod, int ps_flags, const int32_t *d_rnd, size_t Rn, double *d_st,
                             double *d_gst, double *d_out, void *stream) {
    if (int s = grainpool_check(__func__, p, mode, S, T, d_pool, stride, cap, R, d_len, d_slot, overlaps, d_a, d_b, ps_flags, d_st, d_gst,
                                d_out))
        return s;
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    MXG_REQUIRE(p->d_window, "the plan was created without a HIP device");
    if (S == 0 || T == 0) return MXG_OK;
    hipStream_t st = resolve_stream(stream);
    if (d_slot) {
        // a slot index outside the pool is an argument error, refused before anything is launched: the S indices are read back
        // (the one wait of this entry point; a caller that must not wait -- a graph capture -- passes d_slot = NULL)
        std::vector<uint32_t> h_slot(S);
        MXG_HIP(hipMemcpyAsync(h_slot.data(), d_slot, S * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MXG_HIP(hipStreamSynchronize(st));
        if (int s = grainpool_slots_check(__func__, S, R, h_slot.data())) return s;
    }
    int *g_err = nullptr;
    bool err_fresh = false;
    if (int s = scratch_get(SCR_GRAIN_ERR, st, 4 * sizeof(int), (void **)&g_err, &err_fresh)) return s;
    if (err_fresh) MXG_HIP(hipMemsetAsync(g_err, 0, 4 * sizeof(int), st));
    const GpArgs A = grainpool_args(p, p->d_window, S, T, d_pool, stride, cap, R, d_len, d_slot, d_loop, overlaps, d_a, d_b, d_posmod, ps_flags,
                                    d_rnd, Rn, d_st, d_gst, d_out);
    // knob grain_pool_tiles: 0 automatic, 1 the walk only, 2 the tile form wherever it can run
    const int knob = tune_get("grain_pool_tiles");
    const size_t C = (T + kGpTile - 1) / kGpTile;
    const int winPad = (int)((p->sampleDur + 1) & ~(unsigned long)1);
    const size_t tile_lds = sizeof(double) * ((size_t)winPad + (size_t)kGpTile * kGpTilePitch);
    const bool tiles_ok = tile_lds <= 60 * 1024 && C <= 65535 && p->sampleDur < 32768;
    const bool tiles = tiles_ok && (knob == 2 || (knob == 0 && T >= kGpAutoTiles));
    if (tiles) {
        GpLists L;
        L.G = gp_lists_births(T, A.cycleLength);
        L.C = C;
        const size_t nd = 2 * L.G * S + 4 * kGpSlots * S, ni = L.G * S + (C + 1) * S;
        void *scratch = nullptr;
        if (int s = scratch_get(SCR_GRAIN_SCHED, st, nd * sizeof(double) + ni * sizeof(int32_t), &scratch)) return s;
        L.birth_pos = (double *)scratch;
        L.birth_inc = L.birth_pos + L.G * S;
        L.gst_in = L.birth_inc + L.G * S;
        L.birth_n = (int32_t *)(L.gst_in + 4 * kGpSlots * S);
        L.first = L.birth_n + L.G * S;
        const dim3 sgrid((unsigned)((S + 63) / 64));
        {
            KernelTimer kt("grainpool_sched_kernel", st);
            switch (mode) {
                case 0: hipLaunchKernelGGL((grainpool_sched_kernel<0>), sgrid, dim3(64), 0, st, A, L, g_err); break;
                case 1: hipLaunchKernelGGL((grainpool_sched_kernel<1>), sgrid, dim3(64), 0, st, A, L, g_err); break;
                case 2: hipLaunchKernelGGL((grainpool_sched_kernel<2>), sgrid, dim3(64), 0, st, A, L, g_err); break;
                case 3: hipLaunchKernelGGL((grainpool_sched_kernel<3>), sgrid, dim3(64), 0, st, A, L, g_err); break;
                default: hipLaunchKernelGGL((grainpool_sched_kernel<4>), sgrid, dim3(64), 0, st, A, L, g_err); break;
            }
        }
        KernelTimer kt("grainpool_tile_kernel", st);
        hipLaunchKernelGGL(grainpool_tile_kernel, dim3((unsigned)((S + kGpTileStreams - 1) / kGpTileStreams), (unsigned)C), dim3(kGpTileThreads),
                           tile_lds, st, A, L, winPad);
    } else {
        size_t lds = sizeof(double) * p->sampleDur;
        const int winInLds = lds <= 60 * 1024;
        if (!winInLds) lds = 0;
        const dim3 grid((unsigned)((S + 63) / 64));
        KernelTimer kt("grainpool_walk_kernel", st);
        switch (mode) {
            case 0: hipLaunchKernelGGL((grainpool_walk_kernel<0>), grid, dim3(64), lds, st, A, g_err, winInLds); break;
            case 1: hipLaunchKernelGGL((grainpool_walk_kernel<1>), grid, dim3(64), lds, st, A, g_err, winInLds); break;
            case 2: hipLaunchKernelGGL((grainpool_walk_kernel<2>), grid, dim3(64), lds, st, A, g_err, winInLds); break;
            case 3: hipLaunchKernelGGL((grainpool_walk_kernel<3>), grid, dim3(64), lds, st, A, g_err, winInLds); break;
            default: hipLaunchKernelGGL((grainpool_walk_kernel<4>), grid, dim3(64), lds, st, A, g_err, winInLds); break;
        }
    }
    hipLaunchKernelGGL(grainpool_err_publish_kernel, dim3(1), dim3(1), 0, st, g_err, async_error_word());
    return check_hip(hipGetLastError(), "mxg_granular_pool_render launch");
}

int mxg_granular_pool_host(const mxg_grain_plan *p, int mode, size_t S, size_t T, const double *h_pool, size_t stride, size_t cap, size_t R,
                           const uint64_t *h_len, const uint32_t *h_slot, const uint64_t *h_loop, int overlaps, const double *h_a,
                           const double *h_b, const double *h_posmod, int ps_flags, const int32_t *h_rnd, size_t Rn, double *h_st,
                           double *h_gst, double *h_out) {
    if (int s = grainpool_check(__func__, p, mode, S, T, h_pool, stride, cap, R, h_len, h_slot, overlaps, h_a, h_b, ps_flags, h_st, h_gst,
                                h_out))
        return s;
    if (h_slot)
        if (int s = grainpool_slots_check(__func__, S, R, h_slot)) return s;
    if (S == 0 || T == 0) return MXG_OK;
    const GpArgs A = grainpool_args(p, p->h_window.data(), S, T, h_pool, stride, cap, R, h_len, h_slot, h_loop, overlaps, h_a, h_b, h_posmod,
                                    ps_flags, h_rnd, Rn, h_st, h_gst, h_out);
    const int failed = grainpool_host_render(mode, A);
    if (failed) return async_error_status(ASYNC_GRAIN_BASE + failed);  // what the device form reports through the async error word
    return MXG_OK;
}

}  // extern "C"
