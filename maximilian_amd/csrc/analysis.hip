// analysis.hip -- the reference's time-domain analysis classes as voice banks on gfx950 (K16): maxiZeroCrossingDetector,
// maxiZeroCrossingRate, maxiEnvelopeFollower and maxiSampleAndHold (src/maximilian.h:969-1040, 1214-1250).  The per-sample
// arithmetic is mxg_analysis.h, which also compiles for the host (tests/host_analysis.cpp, the drop-in classes).  Compares,
// + - *, integer counts and indexing: bit-exact.
//
// analysis_kernel (mxg_analysis_render) reads the input block [N][V] once and writes any subset of four [N][V] blocks: the
// crossings (0.0 / 1.0), their count over the voice's window, the follower's level and the held sample.  A stage that is not
// asked for does not run and touches neither its state nor its parameters.  The blocks are what mxg_envgen_render (tpv = 1),
// mxg_seq_signal and mxg_dynamics_render (as the control signal) read, so a trigger, a level or a held value is made from the
// audio without a host array in between.
//
// The window of crossings is a ring of BITS, 64 slots to a word, word-major [ceil(cap / 64)][V]: 5.5 KB per voice at 44.1 kHz
// where the reference keeps 353 KB of doubles.  The head and the tail word live in registers; a lane touches the ring once per
// 64 samples (one word written, one or two read).  HBM per sample and voice: 8 B in + 8 B per requested output (+ 8 B for a
// per-sample hold time) + 0.25-0.4 B of ring.
//
// Shape (mxg_stream.h), as envgen.hip / seq.hip: one lane = one voice, chunks of 8 samples, surplus lanes shadow the last voice (pair) and
// store no state, whole chunks leave through emit_chunk (8-byte stores or 16-byte pair rows), the input is requested a chunk
// ahead and consumed before the chunk's stores.  Banks of up to 16 384 voices run in workgroups of one wavefront (dyn.hip), so
// that they still spread over the compute units.  No scratch.
#include "mxg_common.h"
#include "mxg_stream.h"
#include "mxg_analysis.h"

namespace mxg {
namespace {

struct AnaArgs {
    size_t V, N;
    const double *in;  // [N][V]
    int want;          // MXG_ANA_WANT_*
    double *prev_x;    // [V]
    const uint32_t *window;
    uint64_t *zring;  // [ceil(cap / 64)][V]
    int cap;
    int32_t *zpos;
    int64_t *zcount;
    uint32_t *ovf;
    const double *attack, *release;
    double *env;
    const double *hold_ms;
    int hold_ps;  // 1: hold_ms is [N][V]
    double *sah_phase, *sah_value;
    double *o_zx, *o_zcr, *o_env, *o_sah;  // [N][V]
    double sr;
    int px_store;
};

template <bool PX>
__global__ void __launch_bounds__(256) analysis_kernel(AnaArgs A) {
    const size_t V = A.V, N = A.N;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (bank_wave_idle(gid, V)) return;
    const bool live = gid < V;
    const size_t v = bank_voice<PX>(gid, V);
    const int want = A.want;
    const bool w_zcr = (want & MXG_ANA_WANT_ZCR) != 0, w_zx = (want & (MXG_ANA_WANT_ZX | MXG_ANA_WANT_ZCR)) != 0;
    const bool w_env = (want & MXG_ANA_WANT_ENV) != 0, w_sah = (want & MXG_ANA_WANT_SAH) != 0;
    const bool hold_ps = w_sah && A.hold_ps;
    double prev = w_zx ? A.prev_x[v] : 0.0;
    AnaZcr z = {nullptr, V, 1, 1, 0, 0, 0, 0, 0, -1, live};
    uint32_t over = 0;
    if (w_zcr) {
        z.ring = A.zring + v;
        z.cap = A.cap;
        uint32_t w = A.window[v];
        if (w > (uint32_t)A.cap) { w = (uint32_t)A.cap; over = 1; }
        z.window = (int)w;
        const int32_t p = A.zpos[v];
        z.idx = (p >= 0 && p < A.cap) ? p : 0;  // a stored position outside the ring restarts at slot 0
        z.count = A.zcount[v];
        ana_zcr_open(z);
    }
    double att = 0.0, rel = 0.0, env = 0.0;
    if (w_env) { att = A.attack[v]; rel = A.release[v]; env = A.env[v]; }
    double phase = 0.0, held = 0.0, hold = 0.0;
    if (w_sah) {
        phase = A.sah_phase[v];
        held = A.sah_value[v];
        if (!hold_ps) hold = ana_hold_samples(A.hold_ms[v], A.sr);
    }
    constexpr int U = 8;
    const double *__restrict__ ip = A.in + v;
    const double *__restrict__ hp = hold_ps ? A.hold_ms + v : nullptr;
    double xn[U];
    rows_first(xn, ip, V, N);
    // consume every prologue load here (mxg_stream.h)
    asm volatile("" : "+v"(prev), "+v"(att), "+v"(rel), "+v"(env), "+v"(phase), "+v"(held), "+v"(hold), "+v"(z.head), "+v"(z.count));
    double *ozx = (want & MXG_ANA_WANT_ZX) ? A.o_zx + v : nullptr, *ozc = w_zcr ? A.o_zcr + v : nullptr;
    double *oen = w_env ? A.o_env + v : nullptr, *osh = w_sah ? A.o_sah + v : nullptr;
    // one stage after the other over the chunk, each leaving through emit_chunk: one chunk of results is live at a time
    for (size_t n0 = 0; n0 < N; n0 += U) {
        double xc[U], hc[U];
        rows_next(xc, xn, ip, V, N, n0);
        if (hold_ps) {
#pragma unroll
            for (int i = 0; i < U; i++) hc[i] = hp[((n0 + i < N) ? n0 + i : N - 1) * V];
        }
        const int cnt = n0 + U <= N ? U : (int)(N - n0);  // (wave-uniform, mxg_stream.h)
        double y[U];
        unsigned bits = 0;
        if (w_zx) {
#pragma unroll
            for (int i = 0; i < U; i++) {
                const bool bit = ana_zx(prev, xc[i]);
                bits |= (bit ? 1u : 0u) << i;
                y[i] = bit ? 1.0 : 0.0;
                if (i + 1 == cnt) break;
            }
            if (ozx) emit_rows<PX>(ozx, V, y, cnt, A.px_store);
        }
        if (w_zcr) {
#pragma unroll
            for (int i = 0; i < U; i++) {
                y[i] = ana_zcr_step(z, (bits >> i & 1) != 0);
                if (i + 1 == cnt) break;
            }
            emit_rows<PX>(ozc, V, y, cnt, A.px_store);
        }
        if (w_env) {
#pragma unroll
            for (int i = 0; i < U; i++) {
                y[i] = ana_follow<double>(env, att, rel, xc[i]);
                if (i + 1 == cnt) break;
            }
            emit_rows<PX>(oen, V, y, cnt, A.px_store);
        }
        if (w_sah) {
#pragma unroll
            for (int i = 0; i < U; i++) {
                y[i] = ana_sah(phase, held, xc[i], hold_ps ? ana_hold_samples(hc[i], A.sr) : hold);
                if (i + 1 == cnt) break;
            }
            emit_rows<PX>(osh, V, y, cnt, A.px_store);
        }
    }
    if (!live) return;  // a shadow lane owns no state
    if (w_zx) A.prev_x[v] = prev;
    if (w_zcr) {
        ana_zcr_close(z);
        A.zpos[v] = z.idx;
        A.zcount[v] = z.count;
        if (A.ovf && over) A.ovf[v] += over;
    }
    if (w_env) A.env[v] = env;
    if (w_sah) {
        A.sah_phase[v] = phase;
        A.sah_value[v] = held;
    }
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

// maxiEnvelopeFollowerType::setAttack / setRelease (H:1224-1231): the reference's expression with the host libm.
double mxg_envfollow_coeff_host(double ms, double sample_rate) { return pow(0.01, 1.0 / (ms * sample_rate * 0.001)); }

// The host check of a bank's windows before they are uploaded as d_window: a window of 0 samples is refused (the reference would
// subtract the slot its next push overwrites); one above cap passes -- the kernel holds it at cap and counts it in d_overflow.
int mxg_analysis_window_host(size_t V, const uint32_t *h_window, size_t cap) {
    MXG_REQUIRE(h_window, "h_window is null");
    MXG_REQUIRE(cap > 0 && cap <= 0x7fffffff, "cap must be in 1 .. 2^31-1");
    for (size_t v = 0; v < V; v++) MXG_REQUIRE(h_window[v] != 0, "d_window holds a window of 0 samples");
    return MXG_OK;
}

int mxg_analysis_render(size_t V, size_t N, const double *d_in, int want, double *d_prev_x, const uint32_t *d_window,
                        uint64_t *d_zring, size_t cap, int32_t *d_zpos, int64_t *d_zcount, uint32_t *d_overflow,
                        const double *d_attack, const double *d_release, double *d_env, const double *d_hold_ms,
                        int hold_per_sample, double *d_sah_phase, double *d_sah_value, double *d_zx, double *d_zcr,
                        double *d_env_out, double *d_sah, void *stream) {
    MXG_REQUIRE(d_in, "d_in is null");
    MXG_REQUIRE(want != 0, "want selects no output");
    MXG_REQUIRE((want & ~MXG_ANA_WANT_ALL) == 0, "want has an unknown bit");
    if (want & (MXG_ANA_WANT_ZX | MXG_ANA_WANT_ZCR)) MXG_REQUIRE(d_prev_x, "d_prev_x is null (zx, zcr)");
    if (want & MXG_ANA_WANT_ZX) MXG_REQUIRE(d_zx, "d_zx is null");
    if (want & MXG_ANA_WANT_ZCR) {
        MXG_REQUIRE(cap > 0 && cap <= 0x7fffffff, "cap must be in 1 .. 2^31-1");
        MXG_REQUIRE(d_window, "d_window is null");
        MXG_REQUIRE(d_zring, "d_zring is null");
        MXG_REQUIRE(d_zpos, "d_zpos is null");
        MXG_REQUIRE(d_zcount, "d_zcount is null");
        MXG_REQUIRE(d_zcr, "d_zcr is null");
    }
    if (want & MXG_ANA_WANT_ENV) {
        MXG_REQUIRE(d_attack, "d_attack is null");
        MXG_REQUIRE(d_release, "d_release is null");
        MXG_REQUIRE(d_env, "d_env is null");
        MXG_REQUIRE(d_env_out, "d_env_out is null");
    }
    if (want & MXG_ANA_WANT_SAH) {
        MXG_REQUIRE(d_hold_ms, "d_hold_ms is null");
        MXG_REQUIRE(d_sah_phase, "d_sah_phase is null");
        MXG_REQUIRE(d_sah_value, "d_sah_value is null");
        MXG_REQUIRE(d_sah, "d_sah is null");
    }
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    if (V == 0 || N == 0) return MXG_OK;
    hipStream_t st = resolve_stream(stream);
    const int block = voice_block(V, true);
    double *outs[4] = {(want & MXG_ANA_WANT_ZX) ? d_zx : nullptr, (want & MXG_ANA_WANT_ZCR) ? d_zcr : nullptr,
                       (want & MXG_ANA_WANT_ENV) ? d_env_out : nullptr, (want & MXG_ANA_WANT_SAH) ? d_sah : nullptr};
    double *first = nullptr;
    uintptr_t all = 0;
    for (double *o : outs) {
        if (o && !first) first = o;
        all |= (uintptr_t)o;
    }
    int px = rw_store_choice(V, N, first, RW_READ_WRITE);
    if (all & 15) px = 0;
    const AnaArgs A = {V, N, d_in, want, d_prev_x, d_window, d_zring, (int)cap, d_zpos, d_zcount, d_overflow, d_attack, d_release,
                       d_env, d_hold_ms, hold_per_sample ? 1 : 0, d_sah_phase, d_sah_value, outs[0], outs[1], outs[2], outs[3],
                       (double)settings().sampleRate, px};
    KernelTimer kt("analysis_kernel", st);
    with_bools([&](auto PX) { hipLaunchKernelGGL((analysis_kernel<PX.value>), voice_grid(V, block), dim3(block), 0, st, A); }, px != 0);
    return check_hip(hipGetLastError(), "analysis_kernel launch");
}

}  // extern "C"
