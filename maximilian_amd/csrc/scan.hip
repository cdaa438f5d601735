// scan.hip -- SMALL banks of LINEAR recursive filters, parallel in TIME (tolerance mode; knob "time_parallel").
//
// Path: maxiBiquad::play H:1360-1367, maxiSVF::play H:1303-1317, maxiDCBlocker::play H:1261-1266 and maxiFilter::lores / hires
// C:455-484 with block-constant coefficients (hoisted on the host, as in filter2.hip / voice.hip).  The bank kernels give a
// voice to a LANE and walk the block sample by sample: a 6-voice patch (15.polysynth) occupies 6 lanes of one wavefront for
// 512 dependent steps -- 23-28 us of pure latency, however small the bank.  But these filters are linear, time-invariant maps
//      s[n+1] = A s[n] + B x[n],      y[n] = C s[n] + D x[n]            (s: 2-3 doubles per filter)
// so a block can be cut ALONG TIME: a wavefront takes ONE voice, lane k owns the L = N/64 samples [kL, (k+1)L):
//   1. every lane runs its segment from the ZERO state: e_k = the state its inputs alone leave (lane 0 starts from the
//      carried-in state instead, so e_0 is the true state after segment 0);
//   2. M = A^L, the L-step homogeneous transition, is obtained without naming A: lanes 0..2 run the recurrence on the unit
//      states with zero input (the step function is used as a black box), the columns are handed round with readlane
//      (maxiBiquad: in the basis (v2, v1, v1 - v2), see mxg_scan.h);
//   3. the true segment end states obey end_k = M end_{k-1} + e_k: a Kogge-Stone scan over the 64 lanes with wavefront shuffles,
//      q_k += M^(2^j) * shfl_up(q, 2^j), j = 0..5, M^(2^j) by repeated squaring (wave-uniform);
//   4. lane k restarts from end_{k-1} and renders its L samples with the reference's own step, now with the right state.
// 2 L + L recurrence steps and a 6-step scan instead of N dependent steps: a 6-voice x 512-sample block takes a few
// microseconds.  The arithmetic is REORDERED (a state reaches a lane through matrix products instead of through the samples
// before it), so this is a TOLERANCE mode: |error| <= 1e-10 x the voice's peak of the sequential output, for stable settings and
// finite input over the whole parameter domain (measured on the host build, whose bits this kernel must give: <= 6.3e-11 for
// maxiBiquad at 10 Hz and N = 2048 -- the sequential recurrence is itself 3.8e-11 from a long-double one there --, <= 8e-14 for the
// other kinds), stated and tested in tests/test_scan_host.py and tests/test_gpu_scan.py; the default (knob 0) stays the bit-exact
// lane-per-voice kernels.  Used for V <= 4096, N = 64 * {1, 2, 4, 8, 16, 32}.
// The arithmetic -- the steps, the 3x3 algebra, the basis the biquad's scan is carried in, the algorithm above over a lane-exchange
// primitive -- is mxg_scan.h, shared with the host build tests/host_scan.cpp whose bits this kernel must give; here are the
// launches and the wavefront's form of the primitive (__shfl_up, readlane).
#include "mxg_common.h"
#include "mxg_scan.h"

namespace mxg {
namespace {

// the lane-exchange primitive of mxg_scan.h on a wavefront: one lane per executor (W = 1)
__device__ __forceinline__ double bcast(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
struct WaveXch {
    int id;
    __device__ __forceinline__ int lane(int) const { return id; }
    __device__ __forceinline__ void up(const double (&src)[1], int d, double (&dst)[1]) const { dst[0] = __shfl_up(src[0], d); }
    __device__ __forceinline__ double from(const double (&src)[1], int j) const { return bcast(src[0], j); }
};

// one wavefront per voice; NC coefficient rows [NC][V]; state rows st[r * V + v]
template <int KIND, int L>
__global__ __launch_bounds__(64) void scan_filter_kernel(size_t V, size_t N, const double *__restrict__ in,
                                                          const double *__restrict__ coef, double *__restrict__ st,
                                                          double *__restrict__ out) {
    const size_t v = blockIdx.x;
    const int lane = threadIdx.x;
    constexpr int NC = scan_ncoef(KIND), NS = scan_nstate(KIND);
    ScanStep<KIND> step;
#pragma unroll
    for (int r = 0; r < NC; r++) step.c[r] = coef[(size_t)r * V + v];
    const S3 s_in = {st[v], st[V + v], NS == 3 ? st[2 * V + v] : 0.0};
    // this lane's inputs
    double x[1][L];
    const double *ip = in + ((size_t)lane * L) * V + v;
#pragma unroll
    for (int i = 0; i < L; i++) x[0][i] = ip[(size_t)i * V];
    double *op = out + ((size_t)lane * L) * V + v;
    S3 s[1];
    scan_voice<KIND, L, 1>(WaveXch{lane}, step, s_in, x, [&](int, int i, double y) { op[(size_t)i * V] = y; }, s);
    if (lane == 63) {  // (rendered from the scanned start state: the state a following block continues from)
        st[v] = s[0].a;
        st[V + v] = s[0].b;
        if (NS == 3) st[2 * V + v] = s[0].c;
    }
    (void)N;
}

template <int KIND>
int launch_scan(size_t V, size_t N, const double *in, const double *coef, double *st, double *out, hipStream_t s) {
    const dim3 grid((unsigned)V), blk(64);
    switch (N / 64) {
        case 1: hipLaunchKernelGGL((scan_filter_kernel<KIND, 1>), grid, blk, 0, s, V, N, in, coef, st, out); break;
        case 2: hipLaunchKernelGGL((scan_filter_kernel<KIND, 2>), grid, blk, 0, s, V, N, in, coef, st, out); break;
        case 4: hipLaunchKernelGGL((scan_filter_kernel<KIND, 4>), grid, blk, 0, s, V, N, in, coef, st, out); break;
        case 8: hipLaunchKernelGGL((scan_filter_kernel<KIND, 8>), grid, blk, 0, s, V, N, in, coef, st, out); break;
        case 16: hipLaunchKernelGGL((scan_filter_kernel<KIND, 16>), grid, blk, 0, s, V, N, in, coef, st, out); break;
        case 32: hipLaunchKernelGGL((scan_filter_kernel<KIND, 32>), grid, blk, 0, s, V, N, in, coef, st, out); break;
        default: return 1;
    }
    return 0;
}

}  // namespace

// Whether a (V, N) launch takes the time-parallel kernel: the knob, a small bank, a block of 64 * {1, 2, 4, 8, 16, 32} samples.
bool scan_applies(size_t V, size_t N) {
    if (!tune_get("time_parallel")) return false;
    if (V == 0 || V > 4096 || N % 64) return false;
    const size_t L = N / 64;
    return L >= 1 && L <= (size_t)kScanMaxL && (L & (L - 1)) == 0;
}

// kind: 0 maxiDCBlocker, 1 maxiSVF, 2 maxiBiquad (coefficient / state rows as mxg_filter2_render), 3 lores, 4 hires (coef rows c, r;
// state rows x, y of mxg_filter_render's [5][V])
int scan_filter_launch(int kind, size_t V, size_t N, const double *in, const double *coef, double *st, double *out, hipStream_t s) {
    KernelTimer kt("scan_filter_kernel", s);
    int rc = 1;
    switch (kind) {
        case 0: rc = launch_scan<0>(V, N, in, coef, st, out, s); break;
        case 1: rc = launch_scan<1>(V, N, in, coef, st, out, s); break;
        case 2: rc = launch_scan<2>(V, N, in, coef, st, out, s); break;
        case 3: rc = launch_scan<3>(V, N, in, coef, st, out, s); break;
        case 4: rc = launch_scan<4>(V, N, in, coef, st, out, s); break;
    }
    if (rc) return fail(MXG_ERR_INVALID, "scan_filter_launch: unsupported shape");
    return check_hip(hipGetLastError(), "scan_filter_kernel launch");
}

}  // namespace mxg
