// shaper.hip -- the reference's small stream classes as banks on gfx950 (K18): maxiNonlinearity / maxiDistortion
// (src/maximilian.h:1046-1139), maxiXFade (H:1491-1527), maxiSelect / maxiSelectX (H:2018-2088) and maxiLine (H:1532-1617).
// The per-sample arithmetic is mxg_shaper.h, which also compiles for the host (tests/host_shaper.cpp).
//
// shape_kernel, xfade_kernel and select_kernel are the library's first streams without a recurrence over time, so they are FLAT
// over the E = N * V elements of a block instead of one lane per voice: a thread takes 4 units a workgroup's width apart, a unit
// being 16 bytes (two neighbouring elements, whatever rows they are in) where every pointer is 16-byte aligned and the knob
// rw_store is not 1, else one 8-byte element; an odd last element of the 16-byte flavour goes through the 8-byte code of one
// thread.  All loads of a thread are issued before its first store, and a thread reads and writes the same elements, so out ==
// in is allowed.  Per-voice parameters are indexed by element % V: one remainder per thread, then stepped by the (host-computed)
// remainder of the stride.  HBM per element: 8 B in + 8 B out (+ 8 B per per-sample parameter); xfade 8 B + C * 24 B; select
// 8 B index + 8 (Select) or 16 (SelectX) B of values + 8 B out.
//
// line_kernel is a state machine and takes the streaming shape of mxg_stream.h: one lane = one voice, chunks of 8 samples, surplus lanes shadow
// the last voice (pair) and store no state, whole chunks leave through emit_chunk, the trigger is requested a chunk ahead.
// No scratch in any instantiation.  The flat skeleton is mxg_flat.h.
#include <math.h>

#include "mxg_common.h"
#include "mxg_flat.h"
#include "mxg_stream.h"
#include "mxg_shaper.h"

namespace mxg {
namespace {

// ---- maxiNonlinearity ------------------------------------------------------------------------------------------------
struct ShapeArgs {
    FlatGeom g;
    const double *in, *pa, *pb;
    double *out;
};

template <int MODE>
__device__ __forceinline__ double shape_one(double x, double pa, double pb, bool ps) {
    if constexpr (MODE == MXG_SHAPE_ATANDIST) {
        if (ps) pb = shp_atan_norm(pa);  // a shape per sample: the factor is formed here
    }
    return shp_apply<MODE>(x, pa, pb);
}

template <int MODE, bool PS, bool VEC>
__global__ void __launch_bounds__(kFlatBlock) shape_kernel(ShapeArgs A) {
    constexpr int W = VEC ? 2 : 1, R = kFlatUnits;
    constexpr bool NEED_A = MODE >= MXG_SHAPE_FASTATANDIST;
    constexpr bool NEED_B = MODE == MXG_SHAPE_ASYMCLIP || (MODE == MXG_SHAPE_ATANDIST && !PS);
    const size_t E = A.g.E, V = A.g.V;
    const size_t units = VEC ? E >> 1 : E;
    const size_t u0 = (size_t)blockIdx.x * (R * kFlatBlock) + threadIdx.x;
    double x[R][W], pa[R][W], pb[R][W];
    size_t m = (NEED_A && !PS) ? flat_voice0(u0 * W, V) : 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
#pragma unroll
        for (int k = 0; k < W; k++) x[j][k] = pa[j][k] = pb[j][k] = 0.0;
        if (u < units) {
            flat_load<VEC>(A.in, u * W, x[j]);
            if constexpr (NEED_A && PS) flat_load<VEC>(A.pa, u * W, pa[j]);
            if constexpr (NEED_B && PS) flat_load<VEC>(A.pb, u * W, pb[j]);
            if constexpr (NEED_A && !PS) {
                size_t mk = m;
#pragma unroll
                for (int k = 0; k < W; k++) {
                    pa[j][k] = A.pa[mk];
                    if constexpr (NEED_B) pb[j][k] = A.pb[mk];
                    mk = flat_next(mk, 1, V);
                }
            }
        }
        if constexpr (NEED_A && !PS) m = flat_next(m, A.g.stride_mod, V);
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
        if (u < units) {
            double y[W];
#pragma unroll
            for (int k = 0; k < W; k++) y[k] = shape_one<MODE>(x[j][k], pa[j][k], pb[j][k], PS);
            flat_store<VEC>(A.out, u * W, y, A.g.st);
        }
    }
    if (VEC && (E & 1) && u0 == 0) {  // the odd last element of the 16-byte flavour
        const size_t e = E - 1, mv = (NEED_A && !PS) ? e % V : 0;
        const double a = NEED_A ? A.pa[PS ? e : mv] : 0.0, b = NEED_B ? A.pb[PS ? e : mv] : 0.0;
        A.out[e] = shape_one<MODE>(A.in[e], a, b, PS);
    }
}

// ---- maxiXFade -------------------------------------------------------------------------------------------------------
struct XFadeArgs {
    FlatGeom g;
    int C;
    const double *ch1, *ch2, *xf;  // [C][E], [C][E], [E] or [V]
    double *out;                   // [C][E]
};

template <bool PS, bool VEC>
__global__ void __launch_bounds__(kFlatBlock) xfade_kernel(XFadeArgs A) {
    constexpr int W = VEC ? 2 : 1, R = kFlatUnits;
    const size_t E = A.g.E, V = A.g.V;
    const size_t units = VEC ? E >> 1 : E;
    const size_t u0 = (size_t)blockIdx.x * (R * kFlatBlock) + threadIdx.x;
    double g1[R][W], g2[R][W];
    size_t m = PS ? 0 : flat_voice0(u0 * W, V);
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
        double xf[W];
#pragma unroll
        for (int k = 0; k < W; k++) xf[k] = 0.0;
        if (u < units) {
            if constexpr (PS) {
                flat_load<VEC>(A.xf, u * W, xf);
            } else {
                size_t mk = m;
#pragma unroll
                for (int k = 0; k < W; k++) {
                    xf[k] = A.xf[mk];
                    mk = flat_next(mk, 1, V);
                }
            }
        }
        if constexpr (!PS) m = flat_next(m, A.g.stride_mod, V);
#pragma unroll
        for (int k = 0; k < W; k++) shp_xfade_gains(xf[k], g1[j][k], g2[j][k]);  // once, for all C channels
    }
    for (int c = 0; c < A.C; c++) {
        const size_t base = (size_t)c * E;
        double a[R][W], b[R][W];
#pragma unroll
        for (int j = 0; j < R; j++) {
            const size_t u = u0 + (size_t)j * kFlatBlock;
#pragma unroll
            for (int k = 0; k < W; k++) a[j][k] = b[j][k] = 0.0;
            if (u < units) {
                flat_load<VEC>(A.ch1 + base, u * W, a[j]);
                flat_load<VEC>(A.ch2 + base, u * W, b[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < R; j++) {
            const size_t u = u0 + (size_t)j * kFlatBlock;
            if (u < units) {
                double y[W];
#pragma unroll
                for (int k = 0; k < W; k++) y[k] = shp_xfade(a[j][k], b[j][k], g1[j][k], g2[j][k]);
                flat_store<VEC>(A.out + base, u * W, y, A.g.st);
            }
        }
    }
}

// ---- maxiSelect / maxiSelectX ----------------------------------------------------------------------------------------
struct SelectArgs {
    FlatGeom g;
    size_t K;
    int normalised;
    const double *index;   // [E]
    const double *values;  // [K][V] constants or [K][E] signals
    uint32_t *nan_count;   // [V] or null
    double *out;           // [E]
};

template <bool X, bool SIG, bool VEC>
__global__ void __launch_bounds__(kFlatBlock) select_kernel(SelectArgs A) {
    constexpr int W = VEC ? 2 : 1, R = kFlatUnits;
    const size_t E = A.g.E, V = A.g.V, K = A.K;
    const size_t units = VEC ? E >> 1 : E;
    const size_t u0 = (size_t)blockIdx.x * (R * kFlatBlock) + threadIdx.x;
    const size_t plane = SIG ? E : V;  // elements between value k and value k + 1
    const bool normalised = A.normalised != 0;
    double idx[R][W];
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
#pragma unroll
        for (int k = 0; k < W; k++) idx[j][k] = 0.0;
        if (u < units) flat_load<VEC>(A.index, u * W, idx[j]);
    }
    size_t m = flat_voice0(u0 * W, V);
    double y[R][W];
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
        if (u < units) {
            size_t mk = m;
#pragma unroll
            for (int k = 0; k < W; k++) {
                bool nan;
                const double ix = shp_select_index(idx[j][k], K, normalised, &nan);
                if (nan && A.nan_count) atomicAdd(A.nan_count + mk, 1u);
                const size_t col = SIG ? u * W + k : mk;  // (every a below is < K: the index is clamped into [0, K) first)
                if constexpr (X) {
                    size_t a1, a2;
                    double mix;
                    shp_selectx_at(ix, K, a1, a2, mix);
                    y[j][k] = shp_selectx_mix(A.values[a1 * plane + col], A.values[a2 * plane + col], mix);
                } else {
                    y[j][k] = A.values[shp_select_at(ix) * plane + col];
                }
                mk = flat_next(mk, 1, V);
            }
        }
        m = flat_next(m, A.g.stride_mod, V);
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
        if (u < units) flat_store<VEC>(A.out, u * W, y[j], A.g.st);
    }
}

// ---- maxiLine --------------------------------------------------------------------------------------------------------
struct LineArgs {
    size_t V, N;
    double trig_const;
    const double *par;  // [5][V]: lineStart, lineEnd, inc, oneShot, trigEnable
    double *st;         // [4][V]: lineValue, lastTrigVal, triggered, lineComplete
    int px_store;
};

// TB: a trigger block [N][V]; else the constant A.trig_const.  trig / out are separate __restrict__ parameters, as in envgen.hip.
template <bool TB, bool PX>
__global__ void __launch_bounds__(256) line_kernel(LineArgs A, const double *__restrict__ trig_in, double *__restrict__ out_ptr) {
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const bool live = gid < V;
    const size_t v = bank_voice<PX>(gid, V);
    double p_start = A.par[v], p_end = A.par[V + v], p_inc = A.par[2 * V + v], p_one = A.par[3 * V + v], p_en = A.par[4 * V + v];
    double s_value = A.st[v], s_last = A.st[V + v], s_trig = A.st[2 * V + v], s_done = A.st[3 * V + v];
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(p_start), "+v"(p_end), "+v"(p_inc), "+v"(p_one), "+v"(p_en));
    asm volatile("" : "+v"(s_value), "+v"(s_last), "+v"(s_trig), "+v"(s_done));
    const LinePar P = {p_start, p_end, p_inc, p_one != 0.0, p_en != 0.0};
    LineState S = {s_value, s_last, s_trig, s_done != 0.0};
    constexpr int U = 8;
    const double *__restrict__ tp = TB ? trig_in + v : nullptr;
    double *op = out_ptr + v;
    double tn[U];
    if constexpr (TB) rows_first(tn, tp, V, N);
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double tc[U];
        if constexpr (TB) {
            rows_next(tc, tn, tp, V, N, n0);
        } else {
#pragma unroll
            for (int i = 0; i < U; i++) tc[i] = A.trig_const;
        }
        const int cnt = n0 + U <= N ? U : (int)(N - n0);  // (wave-uniform, mxg_stream.h)
        double y[U];
#pragma unroll
        for (int i = 0; i < U; i++) {
            y[i] = shp_line(S, P, tc[i]);
            if (i + 1 == cnt) break;
        }
        emit_rows<PX>(op, V, y, cnt, A.px_store);
    }
    if (!live) return;  // a shadow lane owns no state
    A.st[v] = S.value;
    A.st[V + v] = S.last;
    A.st[2 * V + v] = S.triggered;
    A.st[3 * V + v] = S.complete ? 1.0 : 0.0;
}

template <int MODE>
void shape_launch(bool ps, bool vec, unsigned grid, hipStream_t st, const ShapeArgs &A) {
    with_bools([&](auto PS, auto VEC) {
        hipLaunchKernelGGL((shape_kernel<MODE, PS.value, VEC.value>), dim3(grid), dim3(kFlatBlock), 0, st, A);
    }, ps, vec);
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

// 1.0 / atan(shape) with the host libm: the reference's own factor of atanDist (H:1128), the policy of the filter coefficients.
double mxg_atan_norm_host(double shape) { return 1.0 / atan(shape); }

// maxiLine::prepare (H:1578-1588) on host copies of d_par [5][V] and d_st [4][V], for the voices whose h_mask is non-zero (null:
// every voice): lineValue takes the PREVIOUS lineStart, inc = (end - start) / (ms / 1000.0 * sampleRate), both flags reset.
int mxg_line_prepare_host(size_t V, const double *h_start, const double *h_end, const double *h_ms, const int32_t *h_oneshot,
                          const int32_t *h_mask, double sample_rate, double *h_par, double *h_st) {
    MXG_REQUIRE(h_start, "h_start is null");
    MXG_REQUIRE(h_end, "h_end is null");
    MXG_REQUIRE(h_ms, "h_ms is null");
    MXG_REQUIRE(h_oneshot, "h_oneshot is null");
    MXG_REQUIRE(h_par, "h_par is null");
    MXG_REQUIRE(h_st, "h_st is null");
    for (size_t v = 0; v < V; v++) {
        if (h_mask && !h_mask[v]) continue;
        LineState s = {h_st[v], h_st[V + v], h_st[2 * V + v], h_st[3 * V + v] != 0.0};
        LinePar p = {h_par[v], h_par[V + v], h_par[2 * V + v], h_par[3 * V + v] != 0.0, h_par[4 * V + v] != 0.0};
        shp_line_prepare(s, p, h_start[v], h_end[v], h_ms[v], h_oneshot[v] != 0, sample_rate);
        h_st[v] = s.value; h_st[2 * V + v] = s.triggered; h_st[3 * V + v] = s.complete ? 1.0 : 0.0;
        h_par[v] = p.start; h_par[V + v] = p.end; h_par[2 * V + v] = p.inc; h_par[3 * V + v] = p.oneShot ? 1.0 : 0.0;
    }
    return MXG_OK;
}

int mxg_shape_render(int mode, size_t V, size_t N, const double *d_in, const double *d_a, const double *d_b, int per_sample,
                     double *d_out, void *stream) {
    MXG_REQUIRE(mode >= 0 && mode < MXG_SHAPE_MODES, "mode is not one of MXG_SHAPE_*");
    MXG_REQUIRE(d_in, "d_in is null");
    MXG_REQUIRE(d_out, "d_out is null");
    const bool ps = per_sample != 0;
    if (mode >= MXG_SHAPE_FASTATANDIST) MXG_REQUIRE(d_a, mode == MXG_SHAPE_ASYMCLIP ? "d_a is null (asymclip: a)" : "d_a is null (the shape)");
    if (mode == MXG_SHAPE_ASYMCLIP) MXG_REQUIRE(d_b, "d_b is null (asymclip: b)");
    if (mode == MXG_SHAPE_ATANDIST && !ps) MXG_REQUIRE(d_b, "d_b is null (atanDist per voice: the factors of mxg_atan_norm_host)");
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    if (V == 0 || N == 0) return MXG_OK;
    const bool need_a = mode >= MXG_SHAPE_FASTATANDIST, need_b = mode == MXG_SHAPE_ASYMCLIP || (mode == MXG_SHAPE_ATANDIST && !ps);
    uintptr_t all = (uintptr_t)d_in | (uintptr_t)d_out;
    if (ps && need_a) all |= (uintptr_t)d_a;
    if (ps && need_b) all |= (uintptr_t)d_b;
    bool vec;
    const ShapeArgs A = {flat_geom(V, N, all, &vec), d_in, need_a ? d_a : nullptr, need_b ? d_b : nullptr, d_out};
    const unsigned grid = flat_grid(A.g, vec);
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("shape_kernel", st);
    switch (mode) {
        case MXG_SHAPE_HARDCLIP: shape_launch<MXG_SHAPE_HARDCLIP>(false, vec, grid, st, A); break;
        case MXG_SHAPE_SOFTCLIP: shape_launch<MXG_SHAPE_SOFTCLIP>(false, vec, grid, st, A); break;
        case MXG_SHAPE_FASTATAN: shape_launch<MXG_SHAPE_FASTATAN>(false, vec, grid, st, A); break;
        case MXG_SHAPE_FASTATANDIST: shape_launch<MXG_SHAPE_FASTATANDIST>(ps, vec, grid, st, A); break;
        case MXG_SHAPE_ATANDIST: shape_launch<MXG_SHAPE_ATANDIST>(ps, vec, grid, st, A); break;
        default: shape_launch<MXG_SHAPE_ASYMCLIP>(ps, vec, grid, st, A); break;
    }
    return check_hip(hipGetLastError(), "shape_kernel launch");
}

int mxg_xfade_render(size_t C, size_t V, size_t N, const double *d_ch1, const double *d_ch2, const double *d_xfader,
                     int xfader_per_sample, double *d_out, void *stream) {
    MXG_REQUIRE(C >= 1 && C <= MXG_XFADE_MAX_C, "C must be in 1 .. 8");
    MXG_REQUIRE(d_ch1, "d_ch1 is null");
    MXG_REQUIRE(d_ch2, "d_ch2 is null");
    MXG_REQUIRE(d_xfader, "d_xfader is null");
    MXG_REQUIRE(d_out, "d_out is null");
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    const bool ps = xfader_per_sample != 0;
    uintptr_t all = (uintptr_t)d_ch1 | (uintptr_t)d_ch2 | (uintptr_t)d_out | (ps ? (uintptr_t)d_xfader : 0);
    if ((V * N) & 1) all |= 8;  // an odd block: every second channel starts 8 bytes off -- the 8-byte flavour takes the whole block
    bool vec;
    const XFadeArgs A = {flat_geom(V, N, all, &vec), (int)C, d_ch1, d_ch2, d_xfader, d_out};
    const dim3 grid(flat_grid(A.g, vec)), block(kFlatBlock);
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("xfade_kernel", st);
    with_bools([&](auto PS, auto VEC) { hipLaunchKernelGGL((xfade_kernel<PS.value, VEC.value>), grid, block, 0, st, A); }, ps, vec);
    return check_hip(hipGetLastError(), "xfade_kernel launch");
}

int mxg_select_render(int interpolate, size_t K, size_t V, size_t N, const double *d_index, const double *d_values,
                      int values_are_signals, int normalised, uint32_t *d_nan_count, double *d_out, void *stream) {
    MXG_REQUIRE(K >= 1 && K <= MXG_SELECT_MAX_K, "K must be in 1 .. 64");
    MXG_REQUIRE(d_index, "d_index is null");
    MXG_REQUIRE(d_values, "d_values is null");
    MXG_REQUIRE(d_out, "d_out is null");
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    uintptr_t all = (uintptr_t)d_index | (uintptr_t)d_out;
    if ((V * N) & 1) all |= 8;  // (no odd last element in this kernel: the 8-byte flavour takes the whole block)
    bool vec;
    const SelectArgs A = {flat_geom(V, N, all, &vec), K, normalised ? 1 : 0, d_index, d_values, d_nan_count, d_out};
    const dim3 grid(flat_grid(A.g, vec)), block(kFlatBlock);
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("select_kernel", st);
    with_bools([&](auto X, auto SIG, auto VEC) {
        hipLaunchKernelGGL((select_kernel<X.value, SIG.value, VEC.value>), grid, block, 0, st, A);
    }, interpolate != 0, values_are_signals != 0, vec);
    return check_hip(hipGetLastError(), "select_kernel launch");
}

int mxg_line_render(size_t V, size_t N, const double *d_trig, double trig_const, const double *d_par, double *d_st, double *d_out,
                    void *stream) {
    MXG_REQUIRE(d_par, "d_par is null");
    MXG_REQUIRE(d_st, "d_st is null");
    MXG_REQUIRE(d_out, "d_out is null");
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    const int block = voice_block(V, true);
    const LineArgs A = {V, N, trig_const, d_par, d_st, rw_store_choice(V, N, d_out, d_trig ? RW_READ_WRITE : RW_WRITE_ONLY)};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("line_kernel", st);
    with_bools([&](auto TB, auto PX) {
        hipLaunchKernelGGL((line_kernel<TB.value, PX.value>), voice_grid(V, block), dim3(block), 0, st, A, d_trig, d_out);
    }, d_trig != nullptr, A.px_store != 0);
    return check_hip(hipGetLastError(), "line_kernel launch");
}

}  // extern "C"
