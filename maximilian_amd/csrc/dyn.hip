// dyn.hip -- maxiDynamics and maxiRMS voice banks on gfx950 (K12).
//
// Path (reference src/maximilian.h, cited as H:line): maxiDynamics::play H:2668-2761 over maxiRMS::play H:2604-2610,
// maxiRingBuf H:424-494 and two maxiEnvGen::setupASR envelopes (H:2277-2356, mxg_envgen.h).  The per-sample arithmetic
// is mxg_dyn.h, which also compiles for the host (tests/host_dyn.cpp).  Everything but the two transcendentals --
// log10 in ampToDbs, pow in dbsToAmp -- is + - * / sqrt, compares and integer work: ring contents and positions,
// runningRMS, the envelope state and the positions of NaN / exact 0.0 in the output are the reference's bits unless a
// detector level falls within the device log10's error of a compared boundary; the companded output carries the
// tolerance of DESIGN.md section 4.  sqrt is the correctly rounded one (no fast-math flag on this file).
//
// Shape: one lane = one voice, the block's samples in a serial loop; workgroups of one wavefront, so that a small bank
// still spreads over the compute units.  The stage tables of the two envelopes sit in LDS.  Both rings are slot-major
// ([cap][V]): the lanes of a wavefront whose positions agree touch one row.  The RMS ring's position moves with every
// sample; the look-ahead ring's only where outAmp > 0 (H:2751-2754), so it differs from voice to voice.
// Algorithmic traffic per sample: 8 B in (+ 8 B control when distinct) + 8 B out, RMS ring 8 B write + 8 B tail read,
// look-ahead ring 8 B write + 8 B read.
#include "mxg_common.h"
#include "mxg_dyn.h"

namespace mxg {
namespace {

constexpr int kDynMaxStages = 32;
constexpr int kDynBlock = 64;

__global__ void __launch_bounds__(kDynBlock) dyn_kernel(DynArgs A) {
    __shared__ double s_tab[2][kDynMaxStages * 6];
    for (int i = threadIdx.x; i < A.nstages * 6; i += blockDim.x) {
        s_tab[0][i] = A.tab_h[i];
        s_tab[1][i] = A.tab_l[i];
    }
    __syncthreads();
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= A.V) return;
    dyn_voice_block(A, v, s_tab[0], s_tab[1]);
}

__global__ void __launch_bounds__(kDynBlock) rms_kernel(RmsArgs A) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= A.V) return;
    rms_voice_block(A, v);
}

}  // namespace
}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_dynamics_render(size_t V, size_t N, const double *d_sig, const double *d_control, const double *d_threshold_high,
                        const double *d_ratio_high, const double *d_knee_high, const double *d_threshold_low,
                        const double *d_ratio_low, const double *d_knee_low, int ps_flags, const uint32_t *d_window,
                        const uint32_t *d_lookahead, const int32_t *d_analyser, const double *d_stages_high,
                        const double *d_stages_low, int nstages, double *d_rms_ring, size_t cap_rms, double *d_la_ring,
                        size_t cap_la, int32_t *d_rms_pos, int32_t *d_la_pos, double *d_running, double *d_dst_high,
                        int64_t *d_ist_high, double *d_dst_low, int64_t *d_ist_low, uint32_t *d_overflow, double *d_out,
                        double *d_level_db, void *stream) {
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(d_sig && d_control && d_threshold_high && d_ratio_high && d_knee_high && d_threshold_low && d_ratio_low &&
                    d_knee_low && d_window && d_lookahead && d_analyser && d_stages_high && d_stages_low && d_rms_ring &&
                    d_la_ring && d_rms_pos && d_la_pos && d_running && d_dst_high && d_ist_high && d_dst_low && d_ist_low &&
                    d_out,
                "null device pointer");
    MXG_REQUIRE(cap_rms > 0 && cap_rms <= 0x7fffffff && cap_la > 0 && cap_la <= 0x7fffffff, "ring capacities must be in 1 .. 2^31-1");
    MXG_REQUIRE(nstages >= 1 && nstages <= kDynMaxStages, "nstages out of [1, 32]");
    MXG_REQUIRE((ps_flags & ~MXG_DYN_PS_ALL) == 0, "unknown ps_flags bit");
    if (V == 0 || N == 0) return MXG_OK;
    const DynArgs A = {V, N, d_sig, d_control,
                       {d_threshold_high, d_ratio_high, d_knee_high, d_threshold_low, d_ratio_low, d_knee_low},
                       ps_flags, d_window, d_lookahead, d_analyser, d_stages_high, d_stages_low, nstages,
                       d_rms_ring, (int)cap_rms, d_la_ring, (int)cap_la, d_rms_pos, d_la_pos, d_running,
                       d_dst_high, d_ist_high, d_dst_low, d_ist_low, d_overflow, d_out, d_level_db};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("dyn_kernel", st);
    hipLaunchKernelGGL(dyn_kernel, dim3((unsigned)((V + kDynBlock - 1) / kDynBlock)), dim3(kDynBlock), 0, st, A);
    return check_hip(hipGetLastError(), "dyn_kernel launch");
}

int mxg_rms_render(size_t V, size_t N, const double *d_in, const uint32_t *d_window, double *d_ring, size_t cap,
                   int32_t *d_pos, double *d_running, uint32_t *d_overflow, double *d_out, void *stream) {
    if (int s = ensure_init()) return s;
    MXG_REQUIRE(d_in && d_window && d_ring && d_pos && d_running && d_out, "null device pointer");
    MXG_REQUIRE(cap > 0 && cap <= 0x7fffffff, "cap must be in 1 .. 2^31-1");
    if (V == 0 || N == 0) return MXG_OK;
    const RmsArgs A = {V, N, d_in, d_window, d_ring, (int)cap, d_pos, d_running, d_overflow, d_out};
    hipStream_t st = resolve_stream(stream);
    KernelTimer kt("rms_kernel", st);
    hipLaunchKernelGGL(rms_kernel, dim3((unsigned)((V + kDynBlock - 1) / kDynBlock)), dim3(kDynBlock), 0, st, A);
    return check_hip(hipGetLastError(), "rms_kernel launch");
}

// maxiEnvGen::setTime(index, ms) (H:2449-2462) on one row of a host [nstages][6] table as mxg_envgen_stages_host leaves it.
// Returns 0, or 1 where the reference's setTime reports an error (index out of range, a second HOLD stage).
int mxg_envgen_set_time_host(double *h_stages, size_t nstages, size_t index, double ms) {
    MXG_REQUIRE(h_stages, "null pointer");
    MXG_REQUIRE(nstages >= 1 && nstages <= (size_t)kDynMaxStages, "nstages out of [1, 32]");
    return dyn_envgen_set_time(h_stages, nstages, index, ms, (double)settings().sampleRate);
}

// maxiEnvGen::setLevel (H:2422-2437) / setCurve (H:2440-2446) on a host [nstages][6] table (include/maxigpu.h)
int mxg_envgen_set_level_host(double *h_stages, size_t nstages, size_t index, double value) {
    MXG_REQUIRE(h_stages, "null pointer");
    MXG_REQUIRE(nstages >= 1 && nstages <= (size_t)kDynMaxStages, "nstages out of [1, 32]");
    if (index > nstages) return 1;
    if (index == nstages) {
        h_stages[6 * (index - 1) + 1] = value;
    } else {
        h_stages[6 * index] = value;
        if (index > 0) h_stages[6 * (index - 1) + 1] = value;
    }
    return 0;
}

int mxg_envgen_set_curve_host(double *h_stages, size_t nstages, size_t index, double value) {
    MXG_REQUIRE(h_stages, "null pointer");
    MXG_REQUIRE(nstages >= 1 && nstages <= (size_t)kDynMaxStages, "nstages out of [1, 32]");
    if (index < nstages) h_stages[6 * index + 3] = value;
    return 0;
}

}  // extern "C"
