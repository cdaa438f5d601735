// classic.hip -- the last per-sample classes of the reference's core header as banks on gfx950 (K23): maxiDyn::gate / compressor /
// compress (src/maximilian.cpp:1200-1298), maxiEnvelope::line / trigger (C:377-412), maxiLagExp<double> (src/maximilian.h:499-560),
// maxiMap (H:801-854) and maxiConvert::ampToDbs / dbsToAmp (H:955-961).  The per-sample arithmetic is mxg_classic.h, which also
// compiles for the host (tests/host_classic.cpp and the mxg_*_host entry points below).
//
// dyncls_kernel (gate / compressor), envline_kernel and lag_kernel are state machines and take the streaming shape of
// mxg_stream.h: one lane = one voice, chunks of 8 samples, surplus lanes shadow the last voice (pair) and store no state, whole
// chunks leave through emit_chunk (8-byte stores or 16-byte pair rows, knob rw_store), a ragged last chunk by 8-byte stores, every
// [N][V] input is requested a chunk ahead, the state is read in the prologue and stored once.  A parameter per sample is a second
// instantiation (PS) in which EVERY parameter is a stream with a row stride of V (per sample) or 0 (per voice: the row is re-read,
// it stays in the cache), so that one flag word serves every combination.  HBM per voice and sample: 8 B in + 8 B out (+ 8 B per
// per-sample parameter); the envelope 8 B out (+ 8 B of trigger).
//
// envline_kernel keeps what line() forms from the table -- currentval, sampleRate / period and the two increments -- in registers
// and reloads them where valindex moves to an entry it does not hold (the end of a segment, a trigger; not the end-of-table
// oscillation, which alternates between the entries it holds and an index where nothing is used): the table reads and the
// divisions are off the per-sample path, which is two compares and an add.  Every table index is held inside [0, count - 1] (mxg_classic.h), count itself inside [1, S].
//
// map_kernel is stateless and FLAT over the N * V elements (mxg_flat.h), 16-byte accesses where every pointer allows it; all loads
// of a thread are issued before its first store and a thread reads and writes the same elements, so out == in is allowed.  The
// operand of pow comes from global memory, never from LDS.
// No scratch in any instantiation (.vgpr_spill_count 0).
#include <math.h>

#include "mxg_common.h"
#include "mxg_flat.h"
#include "mxg_stream.h"
#include "mxg_classic.h"

namespace mxg {
namespace {

constexpr int U = 8;  // samples per chunk

// ---- maxiDyn ---------------------------------------------------------------------------------------------------------
struct DynClsArgs {
    size_t V, N;
    const double *thr, *att, *rel, *ratio, *makeup;  // [V], or [N][V] where the stride below is V
    size_t s_thr, s_att, s_rel, s_ratio;             // row strides: V or 0
    const int64_t *holdtime;                         // [V] (gate)
    double *dst;                                     // [3][V]: amplitude, currentRatio, output
    int64_t *ist;                                    // [4][V]: holdcount, attackphase, holdphase, releasephase
    int px_store;
};

// COMP: compressor, else gate.  PS: parameters are streams (see above).  in / out are separate __restrict__ parameters, as in envgen.hip.
template <bool COMP, bool PS, bool PX>
__global__ void __launch_bounds__(256) dyncls_kernel(DynClsArgs A, const double *__restrict__ in_ptr, double *__restrict__ out_ptr) {
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const bool live = gid < V;
    const size_t v = bank_voice<PX>(gid, V);
    double s_amp = A.dst[v], s_cur = A.dst[V + v], s_out = A.dst[2 * V + v];
    int64_t s_hc = A.ist[v], s_ap = A.ist[V + v], s_hp = A.ist[2 * V + v], s_rp = A.ist[3 * V + v];
    int64_t holdtime = COMP ? 0 : A.holdtime[v];
    double p_thr = 0.0, p_att = 0.0, p_rel = 0.0, p_ratio = 0.0, p_mk = 0.0;
    if constexpr (!PS) {
        p_thr = A.thr[v]; p_att = A.att[v]; p_rel = A.rel[v];
        if constexpr (COMP) { p_ratio = A.ratio[v]; p_mk = A.makeup[v]; }
    }
    const double *__restrict__ ip = in_ptr + v;
    const double *__restrict__ tp = A.thr + v, *__restrict__ ap = A.att + v, *__restrict__ rp = A.rel + v;
    const double *__restrict__ qp = COMP ? A.ratio + v : nullptr, *__restrict__ mp = COMP ? A.makeup + v : nullptr;
    double xn[U], tn[U], an[U], rn[U], qn[U], mn[U];
    rows_first(xn, ip, V, N);
    if constexpr (PS) {
        rows_first(tn, tp, A.s_thr, N);
        rows_first(an, ap, A.s_att, N);
        rows_first(rn, rp, A.s_rel, N);
        if constexpr (COMP) {
            rows_first(qn, qp, A.s_ratio, N);
            rows_first(mn, mp, A.s_ratio, N);
        }
    }
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(s_amp), "+v"(s_cur), "+v"(s_out), "+v"(s_hc), "+v"(s_ap), "+v"(s_hp), "+v"(s_rp), "+v"(holdtime));
    asm volatile("" : "+v"(p_thr), "+v"(p_att), "+v"(p_rel), "+v"(p_ratio), "+v"(p_mk));
    ClsDyn S = {s_amp, s_cur, s_out, s_hc, (int)s_ap, (int)s_hp, (int)s_rp};
    double *op = out_ptr + v;
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double xc[U], tc[U], ac[U], rc[U], qc[U], mc[U];
        rows_next(xc, xn, ip, V, N, n0);
        if constexpr (PS) {
            rows_next(tc, tn, tp, A.s_thr, N, n0);
            rows_next(ac, an, ap, A.s_att, N, n0);
            rows_next(rc, rn, rp, A.s_rel, N, n0);
            if constexpr (COMP) {
                rows_next(qc, qn, qp, A.s_ratio, N, n0);
                rows_next(mc, mn, mp, A.s_ratio, N, n0);
            }
        }
        const int cnt = n0 + U <= N ? U : (int)(N - n0);  // (wave-uniform, mxg_stream.h)
        double y[U];
#pragma unroll
        for (int i = 0; i < U; i++) {
            const double thr = PS ? tc[i] : p_thr, att = PS ? ac[i] : p_att, rel = PS ? rc[i] : p_rel;
            if constexpr (COMP) y[i] = cls_compress(S, xc[i], PS ? qc[i] : p_ratio, PS ? mc[i] : p_mk, thr, att, rel);
            else y[i] = cls_gate(S, xc[i], thr, holdtime, att, rel);
            if (i + 1 == cnt) break;
        }
        emit_rows<PX>(op, V, y, cnt, A.px_store);
    }
    if (!live) return;  // a shadow lane owns no state
    A.dst[v] = S.amplitude;
    A.dst[V + v] = S.currentRatio;
    A.dst[2 * V + v] = S.output;
    A.ist[v] = S.holdcount;
    A.ist[V + v] = S.attackphase;
    A.ist[2 * V + v] = S.holdphase;
    A.ist[3 * V + v] = S.releasephase;
}

// ---- maxiEnvelope ----------------------------------------------------------------------------------------------------
struct EnvLineArgs {
    size_t V, N, S;
    const double *seg;          // [S][V]
    const int32_t *count;       // [V]
    const int32_t *trig_index;  // [V] (with a trigger block)
    const double *trig_amp;     // [V]
    double sr;
    double *dst;   // [2][V]: amplitude, startval
    int32_t *ist;  // [2][V]: valindex, isPlaying
    int px_store;
};

// TB: a trigger block [N][V]: a non-zero value performs trigger(trig_index[v], trig_amp[v]) before that sample's line()
template <bool TB, bool PX>
__global__ void __launch_bounds__(256) envline_kernel(EnvLineArgs A, const double *__restrict__ trig_in, double *__restrict__ out_ptr) {
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const bool live = gid < V;
    const size_t v = bank_voice<PX>(gid, V);
    const int n = cls_env_count(A.count[v], A.S);
    const double *__restrict__ seg = A.seg + v;
    int t_index = TB ? A.trig_index[v] : 0;
    double t_amp = TB ? A.trig_amp[v] : 0.0;
    ClsEnv S = {A.dst[v], A.dst[V + v], A.ist[v], A.ist[V + v], 0, 0, 0, 0, MXG_ENV_NONE, 0};
    env_load(S, seg, V, n, A.sr);
    const double *__restrict__ tp = TB ? trig_in + v : nullptr;
    double tn[U];
    if constexpr (TB) rows_first(tn, tp, V, N);
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(S.amplitude), "+v"(S.startval), "+v"(S.valindex), "+v"(S.isPlaying), "+v"(t_index), "+v"(t_amp));
    asm volatile("" : "+v"(S.currentval), "+v"(S.spp), "+v"(S.up), "+v"(S.down));
    double *op = out_ptr + v;
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double tc[U];
        if constexpr (TB) rows_next(tc, tn, tp, V, N, n0);
        const int cnt = n0 + U <= N ? U : (int)(N - n0);  // (wave-uniform, mxg_stream.h)
        double y[U];
#pragma unroll
        for (int i = 0; i < U; i++) {
            if constexpr (TB) {
                if (tc[i] != 0.0) {
                    cls_env_trigger(S, t_index, t_amp, n);
                    env_load(S, seg, V, n, A.sr);
                }
            }
            if (cls_env_line(S, n, y[i])) env_load(S, seg, V, n, A.sr);
            if (i + 1 == cnt) break;
        }
        emit_rows<PX>(op, V, y, cnt, A.px_store);
    }
    if (!live) return;  // a shadow lane owns no state
    A.dst[v] = S.amplitude;
    A.dst[V + v] = S.startval;
    A.ist[v] = S.valindex;
    A.ist[V + v] = S.isPlaying;
}

// ---- maxiLagExp ------------------------------------------------------------------------------------------------------
struct LagArgs {
    size_t V, N;
    const double *alpha, *recip;  // [V], or [N][V] (PS)
    double *val;                  // [V]
    int px_store;
};

template <bool PS, bool PX>
__global__ void __launch_bounds__(256) lag_kernel(LagArgs A, const double *__restrict__ in_ptr, double *__restrict__ out_ptr) {
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const bool live = gid < V;
    const size_t v = bank_voice<PX>(gid, V);
    double val = A.val[v];
    double p_a = PS ? 0.0 : A.alpha[v], p_r = PS ? 0.0 : A.recip[v];
    const double *__restrict__ ip = in_ptr + v;
    const double *__restrict__ ap = A.alpha + v, *__restrict__ rp = A.recip + v;
    double xn[U], an[U], rn[U];
    rows_first(xn, ip, V, N);
    if constexpr (PS) {
        rows_first(an, ap, V, N);
        rows_first(rn, rp, V, N);
    }
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(val), "+v"(p_a), "+v"(p_r));
    double *op = out_ptr + v;
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double xc[U], ac[U], rc[U];
        rows_next(xc, xn, ip, V, N, n0);
        if constexpr (PS) {
            rows_next(ac, an, ap, V, N, n0);
            rows_next(rc, rn, rp, V, N, n0);
        }
        const int cnt = n0 + U <= N ? U : (int)(N - n0);  // (wave-uniform, mxg_stream.h)
        double y[U];
#pragma unroll
        for (int i = 0; i < U; i++) {
            y[i] = val = cls_lag(val, PS ? ac[i] : p_a, PS ? rc[i] : p_r, xc[i]);
            if (i + 1 == cnt) break;
        }
        emit_rows<PX>(op, V, y, cnt, A.px_store);
    }
    if (!live) return;  // a shadow lane owns no state
    A.val[v] = val;
}

// ---- maxiMap / maxiConvert -------------------------------------------------------------------------------------------
struct MapArgs {
    FlatGeom g;
    const double *in, *range, *aux;  // [E], [4][V] (clamp: [2][V]), [V]
    double *out;
};

template <int MODE>
__device__ __forceinline__ void map_params(const MapArgs &A, size_t m, double (&r)[4], double &aux) {
    constexpr int NR = MODE <= MXG_MAP_EXPLIN ? 4 : (MODE == MXG_MAP_CLAMP ? 2 : 0);
#pragma unroll
    for (int q = 0; q < 4; q++) r[q] = q < NR ? A.range[(size_t)q * A.g.V + m] : 0.0;
    aux = MODE == MXG_MAP_EXPLIN ? A.aux[m] : 0.0;
}

template <int MODE, bool VEC>
__global__ void __launch_bounds__(kFlatBlock) map_kernel(MapArgs A) {
    constexpr int W = VEC ? 2 : 1, R = kFlatUnits;
    constexpr bool RANGED = MODE <= MXG_MAP_CLAMP;
    const size_t E = A.g.E, V = A.g.V;
    const size_t units = VEC ? E >> 1 : E;
    const size_t u0 = (size_t)blockIdx.x * (R * kFlatBlock) + threadIdx.x;
    double x[R][W], r[R][W][4], aux[R][W];
    size_t m = RANGED ? flat_voice0(u0 * W, V) : 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
#pragma unroll
        for (int k = 0; k < W; k++) {
            x[j][k] = aux[j][k] = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) r[j][k][q] = 0.0;
        }
        if (u < units) {
            flat_load<VEC>(A.in, u * W, x[j]);
            if constexpr (RANGED) {
                size_t mk = m;
#pragma unroll
                for (int k = 0; k < W; k++) {
                    map_params<MODE>(A, mk, r[j][k], aux[j][k]);
                    mk = flat_next(mk, 1, V);
                }
            }
        }
        if constexpr (RANGED) m = flat_next(m, A.g.stride_mod, V);
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
        const size_t u = u0 + (size_t)j * kFlatBlock;
        if (u < units) {
            double y[W];
#pragma unroll
            for (int k = 0; k < W; k++) y[k] = cls_map<MODE>(x[j][k], r[j][k][0], r[j][k][1], r[j][k][2], r[j][k][3], aux[j][k]);
            flat_store<VEC>(A.out, u * W, y, A.g.st);
        }
    }
    if (VEC && (E & 1) && u0 == 0) {  // the odd last element of the 16-byte flavour
        const size_t e = E - 1;
        double rr[4] = {0.0, 0.0, 0.0, 0.0}, a = 0.0;
        if constexpr (RANGED) map_params<MODE>(A, e % V, rr, a);
        A.out[e] = cls_map<MODE>(A.in[e], rr[0], rr[1], rr[2], rr[3], a);
    }
}

template <int MODE>
void map_launch(bool vec, unsigned grid, hipStream_t st, const MapArgs &A) {
    with_bools([&](auto VEC) { hipLaunchKernelGGL((map_kernel<MODE, VEC.value>), dim3(grid), dim3(kFlatBlock), 0, st, A); }, vec);
}

// the argument checks the device and the host form of the dynamics share
int dyn_check(const char *fn, bool comp, const double *in, const double *ratio, const double *makeup, const double *thr, const double *att,
              const double *rel, int ps_flags, const int64_t *holdtime, const double *dst, const int64_t *ist, const double *out) {
#define CLS_REQ(cond, msg) \
    do { if (!(cond)) return fail(MXG_ERR_INVALID, "%s: %s", fn, msg); } while (0)
    CLS_REQ(in, "the input block is null");
    CLS_REQ(thr, "threshold is null");
    CLS_REQ(att, "attack is null");
    CLS_REQ(rel, "release is null");
    if (comp) {
        CLS_REQ(ratio, "ratio is null");
        CLS_REQ(makeup, "makeup is null (mxg_dyn_makeup_host)");
        CLS_REQ((ps_flags & ~MXG_CLASSIC_PS_MASK) == 0, "ps_flags has an unknown bit");
    } else {
        CLS_REQ(holdtime, "holdtime is null");
        CLS_REQ((ps_flags & ~(MXG_CLASSIC_PS_MASK & ~MXG_CLASSIC_PS_RATIO)) == 0, "ps_flags has an unknown bit (the gate has no ratio)");
    }
    CLS_REQ(dst, "the state array dst is null");
    CLS_REQ(ist, "the state array ist is null");
    CLS_REQ(out, "the output block is null");
    CLS_REQ(out != in, "the output block must be distinct from the input block");
#undef CLS_REQ
    return MXG_OK;
}

int dyn_launch(bool comp, size_t V, size_t N, const double *d_in, const double *d_ratio, const double *d_makeup, const double *d_thr,
               const double *d_att, const double *d_rel, int ps_flags, const int64_t *d_holdtime, double *d_dst, int64_t *d_ist,
               double *d_out, void *stream) {
    const int block = voice_block(V, true);
    const size_t st = (ps_flags & MXG_CLASSIC_PS_THRESHOLD) ? V : 0, sa = (ps_flags & MXG_CLASSIC_PS_ATTACK) ? V : 0;
    const size_t sr = (ps_flags & MXG_CLASSIC_PS_RELEASE) ? V : 0, sq = (ps_flags & MXG_CLASSIC_PS_RATIO) ? V : 0;
    const DynClsArgs A = {V, N, d_thr, d_att, d_rel, d_ratio, d_makeup, st, sa, sr, sq, d_holdtime, d_dst, d_ist,
                          rw_store_choice(V, N, d_out, RW_READ_WRITE)};
    hipStream_t s = resolve_stream(stream);
    KernelTimer kt(comp ? "dyncls_kernel<compress>" : "dyncls_kernel<gate>", s);
    with_bools([&](auto COMP, auto PS, auto PX) {
        hipLaunchKernelGGL((dyncls_kernel<COMP.value, PS.value, PX.value>), voice_grid(V, block), dim3(block), 0, s, A, d_in, d_out);
    }, comp, ps_flags != 0, A.px_store != 0);
    return check_hip(hipGetLastError(), "dyncls_kernel launch");
}

int line_check(const char *fn, size_t S, const double *seg, const int32_t *count, const double *trig, const int32_t *trig_index,
               const double *trig_amp, const double *dst, const int32_t *ist, const double *out) {
#define CLS_REQ(cond, msg) \
    do { if (!(cond)) return fail(MXG_ERR_INVALID, "%s: %s", fn, msg); } while (0)
    CLS_REQ(S >= 2 && S <= MXG_ENVELOPE_MAX_S, "S must be in 2 .. 64");
    CLS_REQ(seg, "the segment tables are null");
    CLS_REQ(count, "count is null");
    if (trig) {
        CLS_REQ(trig_index, "trig_index is null (with a trigger block)");
        CLS_REQ(trig_amp, "trig_amp is null (with a trigger block)");
    }
    CLS_REQ(dst, "the state array dst is null");
    CLS_REQ(ist, "the state array ist is null");
    CLS_REQ(out, "the output block is null");
    CLS_REQ(out != trig, "the output block must be distinct from the trigger block");
#undef CLS_REQ
    return MXG_OK;
}

int map_check(const char *fn, int mode, const double *in, const double *range, const double *aux, const double *out) {
    if (!(mode >= 0 && mode < MXG_MAP_MODES)) return fail(MXG_ERR_INVALID, "%s: mode is not one of MXG_MAP_*", fn);
    if (!in) return fail(MXG_ERR_INVALID, "%s: the input block is null", fn);
    if (!out) return fail(MXG_ERR_INVALID, "%s: the output block is null", fn);
    if (mode <= MXG_MAP_CLAMP && !range) return fail(MXG_ERR_INVALID, "%s: range is null", fn);
    if (mode == MXG_MAP_EXPLIN && !aux) return fail(MXG_ERR_INVALID, "%s: aux is null (explin: mxg_map_range_host)", fn);
    return MXG_OK;
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

// maxiDyn::setAttack / setRelease (C:1300-1306): the reference's expression with the host libm
double mxg_dyn_coeff_host(double ms, double sample_rate) { return cls_dyn_coeff(ms, sample_rate); }

// the compressor's make-up factor 1 + log(ratio) (C:1266) with the host libm
double mxg_dyn_makeup_host(double ratio) { return cls_makeup(ratio); }

// what a map mode needs from the host libm beside its range: explin's log(inMax / inMin) (H:834)
int mxg_map_range_host(int mode, size_t V, const double *h_range, double *h_aux) {
    MXG_REQUIRE(mode >= 0 && mode < MXG_MAP_MODES, "mode is not one of MXG_MAP_*");
    MXG_REQUIRE(h_aux, "h_aux is null");
    if (mode == MXG_MAP_EXPLIN) MXG_REQUIRE(h_range, "h_range is null");
    for (size_t v = 0; v < V; v++) h_aux[v] = mode == MXG_MAP_EXPLIN ? cls_explin_den(h_range[v], h_range[V + v]) : 0.0;
    return MXG_OK;
}

// maxiEnvelope::trigger (C:407-412) on HOST copies of the state arrays, for the voices whose h_mask is non-zero (null: all)
int mxg_envelope_trigger_host(size_t V, const int32_t *h_index, const double *h_amp, const int32_t *h_mask, const int32_t *h_count,
                              double *h_dst, int32_t *h_ist) {
    MXG_REQUIRE(h_index, "h_index is null");
    MXG_REQUIRE(h_amp, "h_amp is null");
    MXG_REQUIRE(h_count, "h_count is null");
    MXG_REQUIRE(h_dst, "h_dst is null");
    MXG_REQUIRE(h_ist, "h_ist is null");
    for (size_t v = 0; v < V; v++) {
        if (h_mask && !h_mask[v]) continue;
        MXG_REQUIRE(h_index[v] >= 0 && h_index[v] <= h_count[v] - 2, "a trigger index is outside [0, count - 2]");
    }
    for (size_t v = 0; v < V; v++) {
        if (h_mask && !h_mask[v]) continue;
        h_ist[V + v] = 1;
        h_ist[v] = h_index[v];
        h_dst[v] = h_amp[v];
    }
    return MXG_OK;
}

int mxg_dyn_gate_render(size_t V, size_t N, const double *d_in, const double *d_threshold, const double *d_attack, const double *d_release,
                        int ps_flags, const int64_t *d_holdtime, double *d_dst, int64_t *d_ist, double *d_out, void *stream) {
    if (int s = dyn_check(__func__, false, d_in, nullptr, nullptr, d_threshold, d_attack, d_release, ps_flags, d_holdtime, d_dst, d_ist, d_out)) return s;
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    if (V == 0 || N == 0) return MXG_OK;
    return dyn_launch(false, V, N, d_in, nullptr, nullptr, d_threshold, d_attack, d_release, ps_flags, d_holdtime, d_dst, d_ist, d_out, stream);
}

int mxg_dyn_gate_host(size_t V, size_t N, const double *h_in, const double *h_threshold, const double *h_attack, const double *h_release,
                      int ps_flags, const int64_t *h_holdtime, double *h_dst, int64_t *h_ist, double *h_out) {
    if (int s = dyn_check(__func__, false, h_in, nullptr, nullptr, h_threshold, h_attack, h_release, ps_flags, h_holdtime, h_dst, h_ist, h_out)) return s;
    cls_host_gate(V, N, h_in, h_threshold, h_attack, h_release, ps_flags, h_holdtime, h_dst, h_ist, h_out);
    return MXG_OK;
}

int mxg_dyn_compress_render(size_t V, size_t N, const double *d_in, const double *d_ratio, const double *d_makeup, const double *d_threshold,
                            const double *d_attack, const double *d_release, int ps_flags, double *d_dst, int64_t *d_ist, double *d_out,
                            void *stream) {
    if (int s = dyn_check(__func__, true, d_in, d_ratio, d_makeup, d_threshold, d_attack, d_release, ps_flags, nullptr, d_dst, d_ist, d_out)) return s;
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    return dyn_launch(true, V, N, d_in, d_ratio, d_makeup, d_threshold, d_attack, d_release, ps_flags, nullptr, d_dst, d_ist, d_out, stream);
}

int mxg_dyn_compress_host(size_t V, size_t N, const double *h_in, const double *h_ratio, const double *h_makeup, const double *h_threshold,
                          const double *h_attack, const double *h_release, int ps_flags, double *h_dst, int64_t *h_ist, double *h_out) {
    if (int s = dyn_check(__func__, true, h_in, h_ratio, h_makeup, h_threshold, h_attack, h_release, ps_flags, nullptr, h_dst, h_ist, h_out)) return s;
    cls_host_compress(V, N, h_in, h_ratio, h_makeup, h_threshold, h_attack, h_release, ps_flags, h_dst, h_ist, h_out);
    return MXG_OK;
}

int mxg_envelope_line_render(size_t V, size_t N, size_t S, const double *d_segments, const int32_t *d_count, const double *d_trig,
                             const int32_t *d_trig_index, const double *d_trig_amp, double *d_dst, int32_t *d_ist, double *d_out,
                             void *stream) {
    if (int s = line_check(__func__, S, d_segments, d_count, d_trig, d_trig_index, d_trig_amp, d_dst, d_ist, d_out)) return s;
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    const int block = voice_block(V, true);
    const EnvLineArgs A = {V, N, S, d_segments, d_count, d_trig_index, d_trig_amp, (double)settings().sampleRate, d_dst, d_ist,
                           rw_store_choice(V, N, d_out, d_trig ? RW_READ_WRITE : RW_WRITE_ONLY)};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("envline_kernel", st);
    with_bools([&](auto TB, auto PX) {
        hipLaunchKernelGGL((envline_kernel<TB.value, PX.value>), voice_grid(V, block), dim3(block), 0, st, A, d_trig, d_out);
    }, d_trig != nullptr, A.px_store != 0);
    return check_hip(hipGetLastError(), "envline_kernel launch");
}

int mxg_envelope_line_host(size_t V, size_t N, size_t S, const double *h_segments, const int32_t *h_count, const double *h_trig,
                           const int32_t *h_trig_index, const double *h_trig_amp, double *h_dst, int32_t *h_ist, double *h_out) {
    if (int s = line_check(__func__, S, h_segments, h_count, h_trig, h_trig_index, h_trig_amp, h_dst, h_ist, h_out)) return s;
    cls_host_line(V, N, S, h_segments, h_count, h_trig, h_trig_index, h_trig_amp, (double)settings().sampleRate, h_dst, h_ist, h_out);
    return MXG_OK;
}

int mxg_lag_render(size_t V, size_t N, const double *d_in, const double *d_alpha, const double *d_alpha_reciprocal, int alpha_per_sample,
                   double *d_val, double *d_out, void *stream) {
    MXG_REQUIRE(d_in, "d_in is null");
    MXG_REQUIRE(d_alpha, "d_alpha is null");
    MXG_REQUIRE(d_alpha_reciprocal, "d_alpha_reciprocal is null");
    MXG_REQUIRE(d_val, "d_val is null");
    MXG_REQUIRE(d_out, "d_out is null");
    MXG_REQUIRE(d_out != d_in, "d_out must be distinct from d_in");
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    const int block = voice_block(V, true);
    const LagArgs A = {V, N, d_alpha, d_alpha_reciprocal, d_val, rw_store_choice(V, N, d_out, RW_READ_WRITE)};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("lag_kernel", st);
    with_bools([&](auto PS, auto PX) {
        hipLaunchKernelGGL((lag_kernel<PS.value, PX.value>), voice_grid(V, block), dim3(block), 0, st, A, d_in, d_out);
    }, alpha_per_sample != 0, A.px_store != 0);
    return check_hip(hipGetLastError(), "lag_kernel launch");
}

int mxg_lag_host(size_t V, size_t N, const double *h_in, const double *h_alpha, const double *h_alpha_reciprocal, int alpha_per_sample,
                 double *h_val, double *h_out) {
    MXG_REQUIRE(h_in, "h_in is null");
    MXG_REQUIRE(h_alpha, "h_alpha is null");
    MXG_REQUIRE(h_alpha_reciprocal, "h_alpha_reciprocal is null");
    MXG_REQUIRE(h_val, "h_val is null");
    MXG_REQUIRE(h_out, "h_out is null");
    cls_host_lag(V, N, h_in, h_alpha, h_alpha_reciprocal, alpha_per_sample, h_val, h_out);
    return MXG_OK;
}

int mxg_map_render(int mode, size_t V, size_t N, const double *d_in, const double *d_range, const double *d_aux, double *d_out, void *stream) {
    if (int s = map_check(__func__, mode, d_in, d_range, d_aux, d_out)) return s;
    if (int s = ensure_init()) return s;
    if (V == 0 || N == 0) return MXG_OK;
    bool vec;
    const MapArgs A = {flat_geom(V, N, (uintptr_t)d_in | (uintptr_t)d_out, &vec), d_in, d_range, d_aux, d_out};
    const unsigned grid = flat_grid(A.g, vec);
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("map_kernel", st);
    switch (mode) {
        case MXG_MAP_LINLIN: map_launch<MXG_MAP_LINLIN>(vec, grid, st, A); break;
        case MXG_MAP_LINEXP: map_launch<MXG_MAP_LINEXP>(vec, grid, st, A); break;
        case MXG_MAP_EXPLIN: map_launch<MXG_MAP_EXPLIN>(vec, grid, st, A); break;
        case MXG_MAP_CLAMP: map_launch<MXG_MAP_CLAMP>(vec, grid, st, A); break;
        case MXG_MAP_AMPTODBS: map_launch<MXG_MAP_AMPTODBS>(vec, grid, st, A); break;
        default: map_launch<MXG_MAP_DBSTOAMP>(vec, grid, st, A); break;
    }
    return check_hip(hipGetLastError(), "map_kernel launch");
}

int mxg_map_host(int mode, size_t V, size_t N, const double *h_in, const double *h_range, const double *h_aux, double *h_out) {
    if (int s = map_check(__func__, mode, h_in, h_range, h_aux, h_out)) return s;
    if (V == 0) return MXG_OK;
    cls_host_map(mode, V, N, h_in, h_range, h_aux, h_out);
    return MXG_OK;
}

}  // extern "C"
