// seq.hip -- the reference's sequencers as voice banks on gfx950 (K15): maxiRatioSeq, maxiStep, maxiCounter, maxiIndex,
// maxiZXToPulse and maxiTrigger::onZX (src/maximilian.h:564-596, 1953-2013, 2093-2262).  The per-sample arithmetic is
// mxg_seq.h, which also compiles for the host (tests/host_seq.cpp).  Compares, + - / floor and integer indexing: bit-exact.
//
// seq_kernel (mxg_seq_render) is the fused sequencer: a clock per voice -- maxiOsc::phasor(freq[v]) with mxg_osc.h's increment
// and recurrence, or a phase signal of the caller's ([N][V] or one shared [N]) -- runs maxiRatioSeq::playTrig against the
// boundary table of the voice's pattern; the trigger feeds playValues or maxiStep::pull over the voice's value list and
// maxiZXToPulse::play.  With the internal clock nothing is read per sample: HBM is 8 B out per sample and output.  The trigger,
// value and gate blocks are what mxg_envgen_render (tpv = 1) and mxg_osc_render (fps = 1) read, so a whole bank is sequenced
// without a host array per block.  seq_signal_kernel (mxg_seq_signal) drives the same step functions from [N][V] signals.
//
// Shape (mxg_stream.h): one lane = one voice, chunks of 8 samples, surplus lanes shadow the last voice (pair), whole chunks leave
// through emit_chunk (8-byte stores or 16-byte pair rows), prologue loads are consumed before the loop, the boundary and value
// tables sit in LDS.  No scratch.
#include "mxg_common.h"
#include "mxg_stream.h"
#include "mxg_seq.h"

namespace mxg {
namespace {

constexpr int kSeqLdsBytes = 48 * 1024;

struct SeqTabs {  // device tables: doubles [P][L] with int32 lengths [P]
    const double *tab;
    const int32_t *len;
    int P, L;
};

struct SeqArgs {
    size_t V, N;
    const double *freq;  // [V], internal clock
    double *clk;         // [V] maxiOsc::phase, in/out
    int phase_pv;        // external phase: 1 = [N][V], 0 = one shared [N]
    SeqTabs pat, val;
    const int32_t *d_pat, *d_vpat;  // [V] or null (= 0)
    const double *step, *hold;      // [V] or null
    double *dst;                    // [5][V]
    int64_t *ist;                   // [6][V]
    double *trig, *valo, *gate;     // [N][V], each optional
    int want;                       // MXG_SEQ_WANT_*
    double sr, inv_sr;
    int px_store;
};

// tables -> LDS: doubles first, then the lengths, held in [1, L]
__device__ __forceinline__ void seq_load_tabs(const SeqTabs &a, const SeqTabs &b, double *s_d, const double *&ta, const double *&tb,
                                              const int *&la, const int *&lb) {
    const int na = a.P * a.L, nb = b.P * b.L;
    int *s_i = reinterpret_cast<int *>(s_d + na + nb);
    for (int i = threadIdx.x; i < na; i += blockDim.x) s_d[i] = a.tab[i];
    for (int i = threadIdx.x; i < nb; i += blockDim.x) s_d[na + i] = b.tab[i];
    for (int i = threadIdx.x; i < a.P; i += blockDim.x) s_i[i] = min(max(a.len[i], 1), a.L);
    for (int i = threadIdx.x; i < b.P; i += blockDim.x) s_i[a.P + i] = min(max(b.len[i], 1), b.L);
    __syncthreads();
    ta = s_d; tb = s_d + na; la = s_i; lb = s_i + a.P;
}
__device__ __forceinline__ int seq_row(const int32_t *sel, size_t v, int P) {  // the voice's table row, held inside the table
    return sel ? min(max(sel[v], 0), P - 1) : 0;
}

// CLK: 0 the internal phasor, 1 an external phase per voice, 2 one shared external phase
template <int CLK, bool PX>
__global__ void __launch_bounds__(256) seq_kernel(SeqArgs A, const double *__restrict__ phase_in) {
    extern __shared__ double s_seq[];
    const double *tpat, *tval;
    const int *lpat, *lval;
    seq_load_tabs(A.pat, A.val, s_seq, tpat, tval, lpat, lval);
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const size_t v = bank_voice<PX>(gid, V);
    const int want = A.want;
    const bool w_val = (want & (MXG_SEQ_WANT_VALUES | MXG_SEQ_WANT_STEP)) != 0, w_step = (want & MXG_SEQ_WANT_STEP) != 0;
    const bool w_gate = (want & MXG_SEQ_WANT_GATE) != 0;
    const int prow = seq_row(A.d_pat, v, A.pat.P);
    const int vrow = w_val ? seq_row(A.d_vpat, v, A.val.P) : 0;
    SeqVoiceCfg c;
    c.bounds = tpat + prow * A.pat.L;
    c.len = lpat[prow];
    c.values = w_val ? tval + vrow * A.val.L : tpat;
    c.vlen = w_val ? lval[vrow] : 1;
    c.step = (w_step && A.step) ? A.step[v] : 1.0;
    c.hold = (w_gate && A.hold) ? A.hold[v] : 0.0;
    c.inv_sr = A.inv_sr;
    c.want = want;
    double clk = 0.0, freq = 0.0;
    if constexpr (CLK == 0) {
        clk = A.clk[v];
        freq = A.freq[v];
    }
    double prevPhase = A.dst[v], sprev = A.dst[V + v], sindex = A.dst[2 * V + v], pprev = A.dst[3 * V + v], phold = A.dst[4 * V + v];
    long long i_rf = A.ist[v], counter = A.ist[V + v], lov = A.ist[2 * V + v];
    long long i_sf = A.ist[3 * V + v], i_sfirst = A.ist[4 * V + v], i_pf = A.ist[5 * V + v];
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(clk), "+v"(freq), "+v"(prevPhase), "+v"(sprev), "+v"(sindex), "+v"(pprev), "+v"(phold));
    asm volatile("" : "+v"(i_rf), "+v"(counter), "+v"(lov), "+v"(i_sf), "+v"(i_sfirst), "+v"(i_pf), "+v"(c.step), "+v"(c.hold));
    SeqRatio r = {prevPhase, i_rf != 0, counter, lov};
    SeqStep st = {{sprev, i_sf != 0}, i_sfirst != 0, sindex};
    SeqPulse pu = {{pprev, i_pf != 0}, phold};
    const OscPre q = osc_pre<MXG_OSC_PHASOR>(freq, A.sr, 0.0, 0.0);
    constexpr int U = 8;
    const double *__restrict__ pp = CLK == 1 ? phase_in + v : phase_in;
    double tn[U];
    if constexpr (CLK == 1) rows_first(tn, pp, V, N);
    double *ot = A.trig ? A.trig + v : nullptr, *ov = w_val ? A.valo + v : nullptr, *og = w_gate ? A.gate + v : nullptr;
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double tc[U];
        if constexpr (CLK == 1) rows_next(tc, tn, pp, V, N, n0);
        const bool whole = n0 + U <= N;  // (wave-uniform; a ragged last chunk goes out sample by sample)
        double xt[U], xv[U], xg[U];
#pragma unroll
        for (int i = 0; i < U; i++) {
            if (n0 + i >= N) break;
            double phase;
            if constexpr (CLK == 0) phase = seq_clock_tick(clk, q);
            else if constexpr (CLK == 1) phase = tc[i];
            else phase = pp[n0 + i];
            double t = 0.0, x = 0.0, g = 0.0;
            seq_voice_tick(r, st, pu, c, phase, t, x, g);
            if (whole) {
                xt[i] = t; xv[i] = x; xg[i] = g;
            } else {
                if (ot) { *ot = t; ot += V; }
                if (ov) { *ov = x; ov += V; }
                if (og) { *og = g; og += V; }
            }
        }
        if (whole) {
            if (ot) emit_chunk<PX>(ot, V, xt, A.px_store);
            if (ov) emit_chunk<PX>(ov, V, xv, A.px_store);
            if (og) emit_chunk<PX>(og, V, xg, A.px_store);
        }
    }
    if constexpr (CLK == 0) A.clk[v] = clk;
    A.dst[v] = r.prevPhase;
    A.ist[v] = r.first ? 1 : 0;
    if (want & MXG_SEQ_WANT_VALUES) {
        A.ist[V + v] = r.counter;
        A.ist[2 * V + v] = r.lengthOfValues;
    }
    if (w_step) {
        A.dst[V + v] = st.trig.prev;
        A.dst[2 * V + v] = st.index;
        A.ist[3 * V + v] = st.trig.first ? 1 : 0;
        A.ist[4 * V + v] = st.first ? 1 : 0;
    }
    if (w_gate) {
        A.dst[3 * V + v] = pu.trig.prev;
        A.dst[4 * V + v] = pu.hold;
        A.ist[5 * V + v] = pu.trig.first ? 1 : 0;
    }
}

struct SigArgs {
    size_t V, N;
    const double *in2;  // COUNTER: the reset signal, INDEX: the index signal
    SeqTabs val;
    const int32_t *d_vpat;
    const double *par;  // [V] STEP: step, ZXTOPULSE: hold time in samples
    double *dst;        // [3][V]
    int64_t *ist;       // [2][V]
    int px_store;
};

template <int KIND, bool PX>
__global__ void __launch_bounds__(256) seq_signal_kernel(SigArgs A, const double *__restrict__ in, double *__restrict__ out) {
    extern __shared__ double s_seq[];
    const double *tval, *tnone;
    const int *lval, *lnone;
    constexpr bool kTab = KIND == MXG_SEQ_STEP || KIND == MXG_SEQ_INDEX;
    constexpr bool kTwo = KIND == MXG_SEQ_COUNTER || KIND == MXG_SEQ_INDEX;
    const SeqTabs none = {nullptr, nullptr, 0, 0};
    seq_load_tabs(kTab ? A.val : none, none, s_seq, tval, tnone, lval, lnone);
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const size_t v = bank_voice<PX>(gid, V);
    const double *values = nullptr;
    int vlen = 1;
    if constexpr (kTab) {
        const int vrow = seq_row(A.d_vpat, v, A.val.P);
        values = tval + vrow * A.val.L;
        vlen = lval[vrow];
    }
    double par = (A.par && (KIND == MXG_SEQ_STEP || KIND == MXG_SEQ_ZXTOPULSE)) ? A.par[v] : (KIND == MXG_SEQ_STEP ? 1.0 : 0.0);
    double d0 = A.dst[v], d1 = A.dst[V + v], d2 = A.dst[2 * V + v];
    long long i0 = A.ist[v], i1 = A.ist[V + v];
    asm volatile("" : "+v"(par), "+v"(d0), "+v"(d1), "+v"(d2), "+v"(i0), "+v"(i1));
    bool f0 = i0 != 0, f1 = i1 != 0;
    constexpr int U = 8;
    const double *ip = in + v, *ip2 = kTwo ? A.in2 + v : nullptr;
    double *op = out + v;
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double a[U], b[U], o[U];
#pragma unroll
        for (int i = 0; i < U; i++) {  // clamped: a ragged last chunk re-reads the block's last row
            const size_t m = (n0 + i < N) ? n0 + i : N - 1;
            a[i] = ip[m * V];
            b[i] = kTwo ? ip2[m * V] : 0.0;
        }
        const bool whole = n0 + U <= N;
#pragma unroll
        for (int i = 0; i < U; i++) {
            if (n0 + i >= N) break;
            double y;
            if constexpr (KIND == MXG_SEQ_ONZX) {
                SeqZx z = {d0, f0};
                y = seq_onzx(z, a[i]);
                d0 = z.prev; f0 = z.first;
            } else if constexpr (KIND == MXG_SEQ_COUNTER) {
                SeqCounter k = {d0, {d1, f0}, {d2, f1}};
                y = seq_counter(k, a[i], b[i]);
                d0 = k.value; d1 = k.inc.prev; f0 = k.inc.first; d2 = k.rst.prev; f1 = k.rst.first;
            } else if constexpr (KIND == MXG_SEQ_STEP) {
                SeqStep s = {{d0, f0}, f1, d1};
                y = seq_step_pull(s, a[i], values, vlen, par);
                d0 = s.trig.prev; f0 = s.trig.first; f1 = s.first; d1 = s.index;
            } else if constexpr (KIND == MXG_SEQ_INDEX) {
                SeqIndex x = {{d0, f0}, d1};
                y = seq_index_pull(x, a[i], b[i], values, vlen);
                d0 = x.trig.prev; f0 = x.trig.first; d1 = x.value;
            } else {
                SeqPulse p = {{d0, f0}, d1};
                y = seq_pulse(p, a[i], par);
                d0 = p.trig.prev; f0 = p.trig.first; d1 = p.hold;
            }
            if (whole) {
                o[i] = y;
            } else {
                *op = y;
                op += V;
            }
        }
        if (whole) emit_chunk<PX>(op, V, o, A.px_store);
    }
    A.dst[v] = d0; A.dst[V + v] = d1; A.dst[2 * V + v] = d2;
    A.ist[v] = f0 ? 1 : 0; A.ist[V + v] = f1 ? 1 : 0;
}

bool tabs_ok(const double *tab, const int32_t *len, size_t P, size_t L) { return tab && len && P >= 1 && L >= 1 && P <= 65536 && L <= 65536; }
size_t tabs_bytes(size_t P, size_t L) { return P * L * sizeof(double) + P * sizeof(int); }

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

// The boundary tables of P patterns of at most L ratios: h_times [P][L] (the first h_len[p] of row p count), h_norm [P][L].
int mxg_seq_ratio_host(size_t P, size_t L, const int32_t *h_len, const double *h_times, double *h_norm) {
    MXG_REQUIRE(h_len && h_times && h_norm, "null pointer");
    MXG_REQUIRE(P >= 1, "no pattern");
    MXG_REQUIRE(L >= 1 && L <= MXG_SEQ_MAX_RATIOS, "L out of [1, 64]");
    for (size_t p = 0; p < P; p++) MXG_REQUIRE(h_len[p] >= 1 && (size_t)h_len[p] <= L, "a pattern's length is out of [1, L]");
    for (size_t p = 0; p < P; p++) seq_ratio_bounds(h_times + p * L, h_len[p], (int)L, h_norm + p * L);
    return MXG_OK;
}

int mxg_seq_render(size_t V, size_t N, const double *d_freq, double *d_clk, const double *d_phase, int phase_pv,
                   const double *d_norm, const int32_t *d_len, size_t P, size_t L, const int32_t *d_pat, int val_mode,
                   const double *d_values, const int32_t *d_vlen, size_t PV, size_t LV, const int32_t *d_vpat,
                   const double *d_step, const double *d_hold, double *d_dst, int64_t *d_ist, double *d_trig, double *d_val,
                   double *d_gate, void *stream) {
    MXG_REQUIRE(d_dst && d_ist, "null state pointer");
    MXG_REQUIRE((d_freq && d_clk && !d_phase) || (!d_freq && !d_clk && d_phase), "give d_freq and d_clk (internal clock) or d_phase (external), not both");
    MXG_REQUIRE(d_norm && d_len && P >= 1, "null pattern table");
    MXG_REQUIRE(L >= 1 && L <= MXG_SEQ_MAX_RATIOS, "L out of [1, 64]");
    MXG_REQUIRE(P <= 65536, "too many patterns");
    MXG_REQUIRE(d_trig || d_val || d_gate, "no output");
    MXG_REQUIRE(val_mode == MXG_SEQ_VAL_VALUES || val_mode == MXG_SEQ_VAL_STEP, "unknown val_mode");
    int want = 0;
    size_t lds = tabs_bytes(P, L);
    SeqTabs vt = {nullptr, nullptr, 0, 0};
    if (d_val) {
        MXG_REQUIRE(tabs_ok(d_values, d_vlen, PV, LV), "d_val needs value lists (d_values, d_vlen, PV >= 1, LV >= 1)");
        want |= val_mode == MXG_SEQ_VAL_STEP ? MXG_SEQ_WANT_STEP : MXG_SEQ_WANT_VALUES;
        vt = {d_values, d_vlen, (int)PV, (int)LV};
        lds += tabs_bytes(PV, LV);
    }
    if (d_gate) want |= MXG_SEQ_WANT_GATE;
    MXG_REQUIRE(lds <= (size_t)kSeqLdsBytes, "pattern and value tables exceed 48 KB");
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    if (V == 0 || N == 0) return MXG_OK;
    const dim3 block(voice_block(V)), grid = voice_grid(V, block.x);
    double *first = d_trig ? d_trig : (d_val ? d_val : d_gate);
    int px = rw_store_choice(V, N, first, RW_WRITE_ONLY);
    if (((uintptr_t)d_trig | (uintptr_t)d_val | (uintptr_t)d_gate) & 15) px = 0;
    const double sr = (double)settings().sampleRate;
    const SeqArgs A = {V, N, d_freq, d_clk, phase_pv, {d_norm, d_len, (int)P, (int)L}, vt, d_pat, d_vpat, d_step, d_hold,
                       d_dst, d_ist, d_trig, d_val, d_gate, want, sr, 1.0 / sr, px};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("seq_kernel", st);
    with_bools([&](auto PX) {
        if (d_freq) hipLaunchKernelGGL((seq_kernel<0, PX.value>), grid, block, lds, st, A, d_phase);
        else if (phase_pv) hipLaunchKernelGGL((seq_kernel<1, PX.value>), grid, block, lds, st, A, d_phase);
        else hipLaunchKernelGGL((seq_kernel<2, PX.value>), grid, block, lds, st, A, d_phase);
    }, px != 0);
    return check_hip(hipGetLastError(), "seq_kernel launch");
}

int mxg_seq_signal(int kind, size_t V, size_t N, const double *d_in, const double *d_in2, const double *d_values,
                   const int32_t *d_vlen, size_t PV, size_t LV, const int32_t *d_vpat, const double *d_par, double *d_dst,
                   int64_t *d_ist, double *d_out, void *stream) {
    MXG_REQUIRE(kind >= MXG_SEQ_ONZX && kind <= MXG_SEQ_ZXTOPULSE, "unknown kind");
    MXG_REQUIRE(d_dst && d_ist, "null state pointer");
    MXG_REQUIRE(d_in && d_out, "null device pointer");
    const bool two = kind == MXG_SEQ_COUNTER || kind == MXG_SEQ_INDEX, tab = kind == MXG_SEQ_STEP || kind == MXG_SEQ_INDEX;
    MXG_REQUIRE(!two || d_in2, "this kind needs a second input signal");
    size_t lds = 0;
    SeqTabs vt = {nullptr, nullptr, 0, 0};
    if (tab) {
        MXG_REQUIRE(tabs_ok(d_values, d_vlen, PV, LV), "this kind needs value lists (d_values, d_vlen, PV >= 1, LV >= 1)");
        vt = {d_values, d_vlen, (int)PV, (int)LV};
        lds = tabs_bytes(PV, LV);
        MXG_REQUIRE(lds <= (size_t)kSeqLdsBytes, "value tables exceed 48 KB");
    }
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    if (V == 0 || N == 0) return MXG_OK;
    const dim3 block(voice_block(V)), grid = voice_grid(V, block.x);
    int px = rw_store_choice(V, N, d_out, RW_READ_WRITE);
    const SigArgs A = {V, N, d_in2, vt, d_vpat, d_par, d_dst, d_ist, px};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("seq_signal_kernel", st);
    with_bools([&](auto PX) {
        switch (kind) {
            case MXG_SEQ_ONZX: hipLaunchKernelGGL((seq_signal_kernel<MXG_SEQ_ONZX, PX.value>), grid, block, lds, st, A, d_in, d_out); break;
            case MXG_SEQ_COUNTER: hipLaunchKernelGGL((seq_signal_kernel<MXG_SEQ_COUNTER, PX.value>), grid, block, lds, st, A, d_in, d_out); break;
            case MXG_SEQ_STEP: hipLaunchKernelGGL((seq_signal_kernel<MXG_SEQ_STEP, PX.value>), grid, block, lds, st, A, d_in, d_out); break;
            case MXG_SEQ_INDEX: hipLaunchKernelGGL((seq_signal_kernel<MXG_SEQ_INDEX, PX.value>), grid, block, lds, st, A, d_in, d_out); break;
            default: hipLaunchKernelGGL((seq_signal_kernel<MXG_SEQ_ZXTOPULSE, PX.value>), grid, block, lds, st, A, d_in, d_out); break;
        }
    }, px != 0);
    return check_hip(hipGetLastError(), "seq_signal_kernel launch");
}

}  // extern "C"
