// kuramoto_wide.hip -- maxiKuramotoOscillatorSet / maxiAsyncKuramotoOscillator (src/maximilian.h:1668-1808) for sets of up to
// 1024 oscillators on gfx950 (K26).  The arithmetic is mxg_kuramoto.h -- the step functions of K17 (kuramoto.hip), unchanged --
// which also compiles for the host (tests/host_kuramoto_wide.cpp): the two agree bit for bit, and for N <= 64 both give
// mxg_kuramoto_render's bits.
//
// kuramoto_wide_kernel (mxg_kuramoto_wide_render): ONE WORKGROUP PER SET, ONE LANE PER OSCILLATOR, 64 * ceil(N / 64) threads.  The
// oscillators of a set are coupled inside every sample and now sit in up to 16 wavefronts, so the exchange through LDS is fenced
// by workgroup barriers: TWO per sample, in every mode, at the top level of the loop over the samples.  Between them the loop
// body has two halves,
//   A (after the first barrier):  every lane publishes what this sample gathers (exact form: its gathered phase; both forms:
//      one word per wavefront saying "all my phases and gathered phases are within |32|"); ONE lane forms the mean-field sums S
//      and C over the sines and cosines published in the last B half; ONE lane of the last wavefront forms the LAST sample's mix.
//   B (after the second barrier): every lane reads the N gathered phases (exact: N sines, all lanes of a wavefront read the same
//      address, an LDS broadcast) or S and C (mean field: one sine / cosine pair), advances, stores, and publishes its new
//      phase for the mix and, in the sync mean-field form, the new phase's sine and cosine for the next sample's sums.
// Every array is written in one half and read in the other, so single buffers do.  The mix of the last sample follows one more
// barrier after the loop.  Nothing inside a branch that only some wavefronts take contains a barrier: those branches are the
// rare accurate reduction behind kura_any and the choice between the trusted and the general sine, which is made from the
// workgroup-wide AND of the per-wavefront words -- a lane reads phases that other wavefronts wrote, so one wavefront's ballot is
// not enough -- and is therefore the same in every wavefront.  The same value feeds the async skip.
//
// Surplus lanes of the last wavefront shadow the set's last oscillator (in slots nobody reads) and store nothing; they run the
// whole loop and every barrier.  LDS: exact 16 KB (gathered, new phases), mean field 24 KB (new phases, sines, cosines).
// HBM per set and sample: as K17.  No scratch.
#include "mxg_common.h"
#include "mxg_kuramoto.h"

namespace mxg {
namespace {

struct KuraWideArgs {
    size_t S, B;
    int N;
    const double *freq, *K;
    int freq_ps, K_ps;  // 1: [B][S]
    double *phase;      // [S][N]
    double *gathered;   // [S][N] (async)
    int32_t *update;    // [S]    (async)
    int want;
    double *mix;         // [B][S]
    double *phases_out;  // [B][S][N]
    double dt;
};

template <bool MF, bool ASYNC>
__global__ void __launch_bounds__(MXG_KURA_WIDE_MAX_N) kuramoto_wide_kernel(KuraWideArgs A) {
    constexpr int W = MXG_KURA_WIDE_MAX_N;
    constexpr bool TRUST = ASYNC || !MF;  // the sync mean-field form takes the general sine / cosine pair and never skips
    __shared__ double s_g[MF ? 1 : W], s_p[W], s_s[MF ? W : 1], s_c[MF ? W : 1], s_sc[2];
    __shared__ int s_ok[64];
    const size_t S = A.S, B = A.B, s = blockIdx.x;
    const int N = A.N;
    const int tid = threadIdx.x, wave = tid >> 6, wl = tid & 63, nw = (int)blockDim.x >> 6;
    const bool live = tid < N;
    const bool mixer = tid == (int)blockDim.x - 64;  // the mix is one lane's, away from the lane that forms S and C
    const int i = live ? tid : N - 1;
    const size_t sn = s * (size_t)N + i;
    double phase = A.phase[sn], gath = phase;
    bool flag = true;  // per set: the same on every lane of the workgroup
    if (ASYNC) {
        gath = A.gathered[sn];
        flag = A.update[s] != 0;
    }
    double si = 0.0, ci = 0.0;
    if (MF) {  // the sines and cosines sample 0 gathers: of the phases, or of an untold async set's stale gathered phases
        kura_sincos<false>(flag ? phase : gath, si, ci);
        s_s[tid] = si;
        s_c[tid] = ci;
    }
    const double *fp = A.freq + s, *kp = A.K + s;
    double fq_n = *fp, k_n = *kp;
    const bool w_mix = (A.want & MXG_KURA_WANT_MIX) != 0, w_ph = (A.want & MXG_KURA_WANT_PHASES) != 0;
    double *om = w_mix ? A.mix + s : nullptr, *op = w_ph ? A.phases_out + sn : nullptr;
    const size_t ostep = S * (size_t)N;
    for (size_t b = 0; b < B; b++) {
        const double fq = fq_n, kk = k_n;
        const size_t bn = b + 1 < B ? b + 1 : b;  // the next sample's parameters, requested a sample ahead
        if (A.freq_ps) fq_n = fp[bn * S];
        if (A.K_ps) k_n = kp[bn * S];
        const bool fl = !ASYNC || (b == 0 && flag);
        __syncthreads();  // ---- half A: the last sample's reads are done, its new phases (and their sines) are visible
        if (w_mix && b > 0 && mixer) {
            *om = kura_mix(s_p, N);
            om += S;
        }
        if (fl) gath = phase;
        if (!MF && (fl || b == 0)) s_g[tid] = gath;
        if (TRUST) {
            const bool trusted = fabs(phase) <= kKuraTrust && fabs(gath) <= kKuraTrust;
            const bool wave_ok = !kura_any(!trusted);
            if (wl == 0) s_ok[wave] = wave_ok ? 1 : 0;
        }
        if (MF && tid == 0 && (!ASYNC || b == 0)) {  // (an async set's gathered phases, and so S and C, stand for the whole call)
            double Ssum, Csum;
            kura_meanfield_sums(s_s, s_c, N, Ssum, Csum);
            s_sc[0] = Ssum;
            s_sc[1] = Csum;
        }
        __syncthreads();  // ---- half B: what this sample gathers is visible
        bool all_trusted = true;
        if (TRUST) all_trusted = !kura_any(wl < nw && s_ok[wl < nw ? wl : 0] == 0);
        const double keff = fl ? kk : 0.0;
        double adj = 0.0;
        const bool skip = ASYNC && !fl && kura_zero_k_skippable(all_trusted, fq);  // the same on every lane of the workgroup
        if (skip) {
            // K is 0 and every term is finite: (0 / N) * adj is a zero that leaves freq as it is
        } else if (MF) {
            if (ASYNC) kura_sincos<false>(phase, si, ci);
            adj = kura_meanfield_adj(si, ci, s_sc[0], s_sc[1]);
        } else {
            adj = all_trusted ? kura_adj_exact<true>(s_g, N, phase) : kura_adj_exact<false>(s_g, N, phase);
        }
        phase = kura_advance(phase, A.dt, fq, keff, N, adj);
        if (w_ph) {
            if (live) *op = phase;
            op += ostep;
        }
        if (w_mix) s_p[tid] = phase;
        if (MF && !ASYNC) {  // what the next sample gathers, and this lane's own pair for it
            kura_sincos<false>(phase, si, ci);
            s_s[tid] = si;
            s_c[tid] = ci;
        }
    }
    __syncthreads();  // (B >= 1: the host launches nothing otherwise)
    if (w_mix && mixer) *om = kura_mix(s_p, N);
    if (!live) return;  // a shadow lane owns no state
    A.phase[sn] = phase;
    if (ASYNC) {
        A.gathered[sn] = gath;
        if (tid == 0) A.update[s] = 0;
    }
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_kuramoto_wide_render(int mode, size_t S, size_t N, size_t B, const double *d_freq, int freq_per_sample, const double *d_K,
                             int K_per_sample, double *d_phase, double *d_gathered, int32_t *d_update, int want, double *d_mix,
                             double *d_phases_out, void *stream) {
    MXG_REQUIRE((mode & ~(MXG_KURA_MEANFIELD | MXG_KURA_ASYNC)) == 0, "mode has an unknown bit");
    MXG_REQUIRE(N >= 1, "N: a set of 0 oscillators");
    MXG_REQUIRE(N <= MXG_KURA_WIDE_MAX_N, "N: a set of more than 1024 oscillators (one workgroup per set is the kernel's scope)");
    MXG_REQUIRE((want & ~(MXG_KURA_WANT_MIX | MXG_KURA_WANT_PHASES)) == 0, "want has an unknown bit");
    MXG_REQUIRE(d_freq, "d_freq is null");
    MXG_REQUIRE(d_K, "d_K is null");
    MXG_REQUIRE(d_phase, "d_phase is null");
    if (mode & MXG_KURA_ASYNC) {
        MXG_REQUIRE(d_gathered, "d_gathered is null (async)");
        MXG_REQUIRE(d_update, "d_update is null (async)");
    }
    if (want & MXG_KURA_WANT_MIX) MXG_REQUIRE(d_mix, "d_mix is null");
    if (want & MXG_KURA_WANT_PHASES) MXG_REQUIRE(d_phases_out, "d_phases_out is null");
    MXG_REQUIRE(S < ((size_t)1 << 31), "2^31 sets or more");
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    if (S == 0 || B == 0) return MXG_OK;
    hipStream_t st = resolve_stream(stream);
    const KuraWideArgs A = {S, B, (int)N, d_freq, d_K, freq_per_sample ? 1 : 0, K_per_sample ? 1 : 0, d_phase, d_gathered, d_update, want,
                            (want & MXG_KURA_WANT_MIX) ? d_mix : nullptr, (want & MXG_KURA_WANT_PHASES) ? d_phases_out : nullptr,
                            MXG_TWOPI / (double)settings().sampleRate};
    const dim3 grid((unsigned)S), block((unsigned)(64 * ((N + 63) / 64)));
    KernelTimer kt("kuramoto_wide_kernel", st);
    switch (mode) {
        case 0: hipLaunchKernelGGL((kuramoto_wide_kernel<false, false>), grid, block, 0, st, A); break;
        case MXG_KURA_MEANFIELD: hipLaunchKernelGGL((kuramoto_wide_kernel<true, false>), grid, block, 0, st, A); break;
        case MXG_KURA_ASYNC: hipLaunchKernelGGL((kuramoto_wide_kernel<false, true>), grid, block, 0, st, A); break;
        default: hipLaunchKernelGGL((kuramoto_wide_kernel<true, true>), grid, block, 0, st, A); break;
    }
    return check_hip(hipGetLastError(), "kuramoto_wide_kernel launch");
}

}  // extern "C"
