// kuramoto.hip -- maxiKuramotoOscillatorSet / maxiAsyncKuramotoOscillator (src/maximilian.h:1628-1808) as banks of coupled
// sets on gfx950 (K17).  The arithmetic is mxg_kuramoto.h, which also compiles for the host (tests/host_kuramoto.cpp): the two
// agree bit for bit.  Everything but the sine keeps the reference's expression trees; the sine is within 1 ULP of glibc's.
//
// kuramoto_kernel (mxg_kuramoto_render): ONE LANE PER OSCILLATOR.  A set of N oscillators (1 .. 64) occupies a segment of
// W = the next power of two >= N lanes, so a wavefront carries 64 / W sets and a workgroup is one wavefront.  The oscillators of
// a set are coupled inside every sample, so each sample the lanes exchange their phases through LDS: every lane writes its
// phase to its slot, then reads the N slots of its segment one after the other -- all lanes of a segment read the same address,
// which LDS serves as a broadcast (one ds_read_b64 per 50 FP64 instructions of the sine that consumes it).  The wavefront runs in
// lockstep and its LDS operations complete in order, so the exchange needs a wavefront-scope fence and no s_barrier; there is no
// traffic between wavefronts at all.  The loop over the B samples is serial: each sample needs the last.
//
// Exact form: N sines per lane and sample, kKuraUnroll independent chains between two branches; the accurate reduction next to a
// zero of the sine is one wave-uniform branch per group.  Mean-field form: one sine / cosine pair per lane, two more slots per
// lane, 2 N additions.  Lanes whose phases are all within |32| (a ballot per sample) take the range-test-free sine; a wavefront
// with a stray or non-finite phase takes the general one, one term at a time.
//
// Surplus lanes of a segment shadow the set's last oscillator (in a slot nobody reads), surplus segments of the last wavefront
// shadow the last set; neither stores anything.  HBM per set and sample: 8 B of mix, 8 N B of phases_out, 8 B each of a
// per-sample freq / K; the state (8 N B, async 16 N + 4 B) moves once per launch.  No scratch.
#include "mxg_common.h"
#include "mxg_kuramoto.h"

namespace mxg {
namespace {

struct KuraArgs {
    size_t S, B;
    int N, wlog;  // W = 1 << wlog
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

// what one lane wrote to LDS is visible to the other lanes of its wavefront (which runs in lockstep; LDS operations of a
// wavefront complete in order): a compiler fence + the wave barrier pseudo-instruction, no s_barrier
__device__ __forceinline__ void kura_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool MF, bool ASYNC>
__global__ void __launch_bounds__(64) kuramoto_kernel(KuraArgs A) {
    __shared__ double s_g[64], s_p[64], s_s[MF ? 64 : 1], s_c[MF ? 64 : 1];
    const size_t S = A.S, B = A.B;
    const int N = A.N, W = 1 << A.wlog;
    const int lane = threadIdx.x;
    const size_t set0 = (size_t)blockIdx.x << (6 - A.wlog);  // first set of this wavefront
    if (set0 >= S) return;
    const int seg = lane >> A.wlog, i0 = lane & (W - 1), base = seg << A.wlog;
    const size_t sraw = set0 + seg;
    const bool live = sraw < S && i0 < N;
    const size_t s = sraw < S ? sraw : S - 1;
    const int i = i0 < N ? i0 : N - 1;
    const size_t sn = s * (size_t)N + i;
    double phase = A.phase[sn];
    const double *g = s_g + base, *p = s_p + base;
    bool flag = true;
    double gsin = 0.0, gcos = 0.0;
    if (ASYNC) {
        s_g[lane] = A.gathered[sn];
        flag = A.update[s] != 0;
        if (MF && !flag) {  // the sines and cosines of the stale gathered phases
            kura_sincos<false>(s_g[lane], gsin, gcos);
            s_s[lane] = gsin;
            s_c[lane] = gcos;
        }
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
        kura_lds_sync();  // (the last sample's reads are done)
        if (fl) s_g[lane] = phase;
        bool trusted = fabs(phase) <= kKuraTrust;
        if (ASYNC) trusted = trusted && fabs(s_g[lane]) <= kKuraTrust;
        const bool all_trusted = !kura_any(!trusted);
        const double keff = fl ? kk : 0.0;
        double adj = 0.0;
        const bool skip = ASYNC && !kura_any(fl || !kura_zero_k_skippable(all_trusted, fq));
        if (skip) {
            // K is 0 and every term is finite: (0 / N) * adj is a zero that leaves freq as it is
        } else if (MF) {
            double si, ci;
            kura_sincos<false>(phase, si, ci);
            if (fl) {
                s_s[lane] = si;
                s_c[lane] = ci;
            }
            kura_lds_sync();
            adj = kura_adj_meanfield(s_s + base, s_c + base, N, si, ci);
        } else {
            kura_lds_sync();
            adj = all_trusted ? kura_adj_exact<true>(g, N, phase) : kura_adj_exact<false>(g, N, phase);
        }
        phase = kura_advance(phase, A.dt, fq, keff, N, adj);
        if (w_ph) {
            if (live) *op = phase;
            op += ostep;
        }
        if (w_mix) {
            s_p[lane] = phase;
            kura_lds_sync();
            const double mix = kura_mix(p, N);
            if (live && i0 == 0) *om = mix;
            om += S;
        }
    }
    if (!live) return;  // a shadow lane owns no state
    A.phase[sn] = phase;
    if (ASYNC) {
        A.gathered[sn] = s_g[lane];
        if (i0 == 0) A.update[s] = 0;
    }
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_kuramoto_render(int mode, size_t S, size_t N, size_t B, const double *d_freq, int freq_per_sample, const double *d_K,
                        int K_per_sample, double *d_phase, double *d_gathered, int32_t *d_update, int want, double *d_mix,
                        double *d_phases_out, void *stream) {
    MXG_REQUIRE((mode & ~(MXG_KURA_MEANFIELD | MXG_KURA_ASYNC)) == 0, "mode has an unknown bit");
    MXG_REQUIRE(N >= 1, "a set of 0 oscillators");
    MXG_REQUIRE(N <= MXG_KURA_MAX_N, "a set of more than 64 oscillators (one wavefront per set is the kernel's scope)");
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
    int wlog = 0;
    while (((size_t)1 << wlog) < N) wlog++;
    const size_t per_wave = (size_t)64 >> wlog;
    const KuraArgs A = {S, B, (int)N, wlog, d_freq, d_K, freq_per_sample ? 1 : 0, K_per_sample ? 1 : 0, d_phase, d_gathered, d_update,
                        want, (want & MXG_KURA_WANT_MIX) ? d_mix : nullptr, (want & MXG_KURA_WANT_PHASES) ? d_phases_out : nullptr,
                        MXG_TWOPI / (double)settings().sampleRate};
    const dim3 grid((unsigned)((S + per_wave - 1) / per_wave)), block(64);
    KernelTimer kt("kuramoto_kernel", st);
    switch (mode) {
        case 0: hipLaunchKernelGGL((kuramoto_kernel<false, false>), grid, block, 0, st, A); break;
        case MXG_KURA_MEANFIELD: hipLaunchKernelGGL((kuramoto_kernel<true, false>), grid, block, 0, st, A); break;
        case MXG_KURA_ASYNC: hipLaunchKernelGGL((kuramoto_kernel<false, true>), grid, block, 0, st, A); break;
        default: hipLaunchKernelGGL((kuramoto_kernel<true, true>), grid, block, 0, st, A); break;
    }
    return check_hip(hipGetLastError(), "kuramoto_kernel launch");
}

}  // extern "C"
