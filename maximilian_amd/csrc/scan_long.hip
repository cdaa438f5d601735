// scan_long.hip -- K28: LINEAR recursive filters over LONG signals of FEW voices, parallel in TIME (mxg_scan_long_render).
//
// Path: maxiBiquad::play H:1360-1367, maxiSVF::play H:1303-1317, maxiDCBlocker::play H:1261-1266, maxiFilter::lores / hires
// C:455-484 and maxiLagExp<double>::addSample H:523-556, block-constant coefficients.  The lane-per-voice kernels walk a signal
// sample by sample on one lane; K10 (scan.hip) cuts a block of up to 2048 samples along time on ONE wavefront.  Here a voice's
// signal is cut into chunks of T = 2048 samples and the chunks are joined by a second scan, in three launches on the caller's
// stream (the arithmetic, the decomposition of N and the host twin whose bits these kernels must give: mxg_scan_long.h):
//   A. scan_long_summary_kernel   one wavefront per (chunk, voice), chunks 0 .. C-2: the state the chunk's inputs leave from zero
//                                 (chunk 0: from the carried-in state), 3 doubles to scratch;
//   B. scan_long_chunks_kernel    one wavefront per voice: the scan over the chunks, the true state after every chunk to scratch;
//   C. scan_long_render_kernel    one wavefront per (chunk, voice): K10's scan_voice from the chunk's start state, the outputs; the
//                                 last chunk's wavefront renders the remainder (< 2048 samples) and stores the carried state.
// No workgroup waits on another: the order between the phases is stream order between launches, and there are no atomics.  Scratch
// (SCR_SCAN_LONG, per stream, grow-only): summaries and states, [V][C-1][3] doubles each -- voice-major, so that the lane of phase B
// that walks a run of consecutive chunks walks consecutive memory -- and [V][3] for the carried-in state, which phase A copies so
// that in phase C no workgroup reads the state array another one writes.
//
// Memory.  K10's lane k reads in[(k L + i) V + v]: neighbouring lanes are L V doubles apart.  At millions of samples that decides
// the time, so phases A and C stage the chunk through LDS: the workgroup reads its (2048 samples x G voices) tile with consecutive
// threads on consecutive addresses (runs of G doubles per row of the [N][V] layout; the whole row when V <= G), writes it to LDS
// with the segment stride padded from 32 to 33 doubles, and lane k reads its 32 samples at 33 k + i: ds_read_b64, the 32 lanes of a
// half on 32 distinct 8-byte banks.  The staging writes are consecutive doubles within each 16-lane group (G = 4: the voices' images
// are 4 doubles apart mod 16), conflict-free as well.  Phase C writes its outputs to the lane's own segment of the same image (its
// inputs are in registers by then) and the workgroup stores the tile as it loaded it, so out == in works: a workgroup reads and
// writes its own tile only, and phase A has finished before phase C starts.  Algorithmic traffic: 8 B read in A, 8 B read and 8 B
// written in C per voice-sample; the summaries are 48 B per 2048 samples.
//
// Workgroups.  G = 1 wavefront (V = 1: 16.5 KiB of LDS) or G = 4 wavefronts, each owning one voice of the same chunk (V >= 2: 66 KiB).
// scan_voice at L = 32 holds 32 inputs and the scan in registers (over 128 VGPRs: at most 3 wavefronts per SIMD anyway), so LDS is
// not what bounds occupancy: 160 KiB per CU hold 9 workgroups of G = 1 or 2 of G = 4 (8 wavefronts, 2 per SIMD), and the loads of a
// tile are all issued before the first wait.  Wider workgroups at G = 8 would take 132 KiB and leave one workgroup per CU with
// nothing to overlap its barrier; narrower ones shorten the contiguous runs of the global accesses.  (The runs of 32 B at V > 4 share
// their 128-B lines with the neighbouring workgroups of the same chunk, which run at the same time: the L2 serves them.)
#include "mxg_common.h"
#include "mxg_scan_long.h"

namespace mxg {
namespace {

constexpr int kSegStride = kScanMaxL + 1;                   // a lane's 32 samples, padded: lane k at 33 k
constexpr int kTileStride = kScanLanes * kSegStride + 4;    // one voice's image; + 4: the G images 4 doubles apart mod 16
constexpr size_t kLongMaxV = 4096, kLongMaxN = (size_t)1 << 28;

__device__ __forceinline__ double bcast(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
struct WaveXch {  // the lane-exchange primitive of mxg_scan.h on a wavefront: one lane per executor (W = 1)
    int id;
    __device__ __forceinline__ int lane(int) const { return id; }
    __device__ __forceinline__ void up(const double (&src)[1], int d, double (&dst)[1]) const { dst[0] = __shfl_up(src[0], d); }
    __device__ __forceinline__ double from(const double (&src)[1], int j) const { return bcast(src[0], j); }
};

__device__ __forceinline__ int tile_at(int t) { return t + (t >> 5); }  // sample t of a chunk in a voice's image

// the workgroup's tile, rows [t0, t0 + 2048) x voices [v0, v0 + G) of an [N][V] array, global <-> LDS; consecutive threads on consecutive addresses
template <int G>
__device__ __forceinline__ void tile_load(double *tile, const double *base, size_t V, size_t v0, int tid) {
#pragma unroll 8
    for (int f = tid; f < kLongChunk * G; f += kScanLanes * G) {
        const int t = f / G, g = f % G;
        if (v0 + g < V) tile[g * kTileStride + tile_at(t)] = base[(size_t)t * V + v0 + g];
    }
}
template <int G>
__device__ __forceinline__ void tile_store(const double *tile, double *base, size_t V, size_t v0, int tid) {
#pragma unroll 8
    for (int f = tid; f < kLongChunk * G; f += kScanLanes * G) {
        const int t = f / G, g = f % G;
        if (v0 + g < V) base[(size_t)t * V + v0 + g] = tile[g * kTileStride + tile_at(t)];
    }
}

template <int KIND>
__device__ __forceinline__ ScanStep<KIND> load_step(const double *__restrict__ coef, size_t V, size_t v) {
    ScanStep<KIND> step;
#pragma unroll
    for (int r = 0; r < scan_long_ncoef(KIND); r++) step.c[r] = coef[(size_t)r * V + v];
    return step;
}
template <int KIND>
__device__ __forceinline__ S3 load_state(const double *st, size_t V, size_t v) {
    constexpr int NS = scan_long_nstate(KIND);
    return S3{st[v], NS >= 2 ? st[V + v] : 0.0, NS == 3 ? st[2 * V + v] : 0.0};
}

// A: grid (K, ceil(V / G)), chunk c = blockIdx.x < K = C - 1; sum [V][K][3]; start0 [V][3]: the carried-in state, copied by chunk 0's
// wavefront for phase C -- whose last workgroup writes st while its first would otherwise still have to read it
template <int KIND, int G>
__global__ __launch_bounds__(64 * G) void scan_long_summary_kernel(size_t V, size_t K, const double *__restrict__ in,
                                                                    const double *__restrict__ coef, const double *__restrict__ st,
                                                                    double *__restrict__ sum, double *__restrict__ start0) {
    extern __shared__ double tile[];
    const size_t c = blockIdx.x, v0 = (size_t)blockIdx.y * G;
    const int tid = threadIdx.x, g = tid / kScanLanes, lane = tid % kScanLanes;
    tile_load<G>(tile, in + c * kLongChunk * V, V, v0, tid);
    __syncthreads();
    const size_t v = v0 + g;
    if (v >= V) return;
    const ScanStep<KIND> step = load_step<KIND>(coef, V, v);
    const S3 s_in = c == 0 ? load_state<KIND>(st, V, v) : S3{0.0, 0.0, 0.0};
    double x[1][kScanMaxL];
    const double *seg = tile + g * kTileStride + lane * kSegStride;
#pragma unroll
    for (int i = 0; i < kScanMaxL; i++) x[0][i] = seg[i];
    const S3 e = scan_summary<KIND, kScanMaxL, 1>(WaveXch{lane}, step, c == 0, s_in, x);
    if (lane == 0) {
        double *o = sum + (v * K + c) * 3;
        o[0] = e.a, o[1] = e.b, o[2] = e.c;
        if (c == 0) start0[3 * v] = s_in.a, start0[3 * v + 1] = s_in.b, start0[3 * v + 2] = s_in.c;
    }
}

// B: grid V, one wavefront per voice; sum -> ends, both [V][K][3]
template <int KIND>
__global__ __launch_bounds__(64) void scan_long_chunks_kernel(size_t V, size_t K, const double *__restrict__ coef,
                                                               const double *__restrict__ sum, double *__restrict__ ends) {
    const size_t v = blockIdx.x;
    const int lane = threadIdx.x;
    const ScanStep<KIND> step = load_step<KIND>(coef, V, v);
    const WaveXch xch{lane};
    const M3 MT = scan_chunk_transition<KIND, 1>(xch, step);
    const double *e = sum + v * K * 3;
    double *E = ends + v * K * 3;
    scan_chunks<1>(xch, MT, K, [&](size_t c) { return S3{e[3 * c], e[3 * c + 1], e[3 * c + 2]}; },
                   [&](size_t c, const S3 &q) { E[3 * c] = q.a, E[3 * c + 1] = q.b, E[3 * c + 2] = q.c; });
}

// C: grid (max(C, 1), ceil(V / G)); ends [V][K][3] and start0 [V][3], K = C - 1 (unused when C <= 1); R = N % 2048.  st is read only
// when C <= 1, by the one workgroup of the voice that also writes it
template <int KIND, int G>
__global__ __launch_bounds__(64 * G) void scan_long_render_kernel(size_t V, size_t C, size_t R, const double *in,
                                                                   const double *__restrict__ coef, double *__restrict__ st,
                                                                   const double *__restrict__ ends, const double *__restrict__ start0,
                                                                   double *out) {
    extern __shared__ double tile[];
    const size_t c = blockIdx.x, v0 = (size_t)blockIdx.y * G;
    const int tid = threadIdx.x, g = tid / kScanLanes, lane = tid % kScanLanes;
    const size_t v = v0 + g;
    const bool live = v < V, chunk = c < C, last = c + 1 >= C;  // (chunk and last are the same in the whole workgroup)
    const WaveXch xch{lane};
    ScanStep<KIND> step;
    S3 s = {0.0, 0.0, 0.0};
    if (live) {
        step = load_step<KIND>(coef, V, v);
        if (c == 0) s = C >= 2 ? S3{start0[3 * v], start0[3 * v + 1], start0[3 * v + 2]} : load_state<KIND>(st, V, v);
        else {
            const double *E = ends + (v * (C - 1) + (c - 1)) * 3;
            s = scan_restart<KIND>(S3{E[0], E[1], E[2]});
        }
    }
    if (chunk) {
        tile_load<G>(tile, in + c * kLongChunk * V, V, v0, tid);
        __syncthreads();
        if (live) {
            double *seg = tile + g * kTileStride + lane * kSegStride;
            s = scan_block<KIND, kScanMaxL, 1>(xch, step, s, [&](int, size_t n) { return seg[n - (size_t)lane * kScanMaxL]; },
                                               [&](int, size_t n, double y) { seg[n - (size_t)lane * kScanMaxL] = y; });
        }
        __syncthreads();
        tile_store<G>(tile, out + c * kLongChunk * V, V, v0, tid);
    }
    if (!live || !last) return;
    const size_t n0 = C * kLongChunk;  // the remainder: straight from global memory, every load of a block before its first store
    const double *ip = in + n0 * V + v;
    double *op = out + n0 * V + v;
    s = scan_tail<KIND, 1>(xch, step, s, R, [&](int, size_t n) { return ip[n * V]; }, [&](int, size_t n, double y) { op[n * V] = y; },
                           [&](size_t n) { return ip[n * V]; }, [&](size_t n, double y) { if (lane == 0) op[n * V] = y; });
    if (lane == 0) {
        constexpr int NS = scan_long_nstate(KIND);
        st[v] = s.a;
        if (NS >= 2) st[V + v] = s.b;
        if (NS == 3) st[2 * V + v] = s.c;
    }
}

template <int G>
constexpr size_t tile_bytes() { return (size_t)G * kTileStride * sizeof(double); }

template <int KIND, int G>
int launch_long(size_t V, size_t N, const double *in, const double *coef, double *st, double *out, hipStream_t s) {
    const size_t C = N / kLongChunk, K = C > 1 ? C - 1 : 0, R = N % kLongChunk;
    const size_t groups = (V + G - 1) / G;
    constexpr size_t lds = tile_bytes<G>();
    if (lds > 64 * 1024) {  // (once per kernel: above 64 KiB of LDS a kernel has to be told)
        static const hipError_t ea = hipFuncSetAttribute((const void *)scan_long_summary_kernel<KIND, G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        static const hipError_t ec = hipFuncSetAttribute((const void *)scan_long_render_kernel<KIND, G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        MXG_HIP(ea);
        MXG_HIP(ec);
    }
    double *sum = nullptr, *ends = nullptr, *start0 = nullptr;
    if (K) {
        void *p = nullptr;
        if (int rc = scratch_get(SCR_SCAN_LONG, s, (2 * K + 1) * V * 3 * sizeof(double), &p)) return rc;
        sum = (double *)p;
        ends = sum + K * V * 3;
        start0 = ends + K * V * 3;
        {
            KernelTimer kt("scan_long_summary_kernel", s);
            hipLaunchKernelGGL((scan_long_summary_kernel<KIND, G>), dim3((unsigned)K, (unsigned)groups), dim3(64 * G), lds, s, V, K, in, coef, st, sum, start0);
        }
        MXG_HIP(hipGetLastError());
        {
            KernelTimer kt("scan_long_chunks_kernel", s);
            hipLaunchKernelGGL((scan_long_chunks_kernel<KIND>), dim3((unsigned)V), dim3(64), 0, s, V, K, coef, sum, ends);
        }
        MXG_HIP(hipGetLastError());
    }
    {
        KernelTimer kt("scan_long_render_kernel", s);
        hipLaunchKernelGGL((scan_long_render_kernel<KIND, G>), dim3((unsigned)(C ? C : 1), (unsigned)groups), dim3(64 * G), lds, s, V, C, R, in, coef, st, ends, start0, out);
    }
    return check_hip(hipGetLastError(), "scan_long_render_kernel launch");
}

template <int KIND>
int launch_long_g(size_t V, size_t N, const double *in, const double *coef, double *st, double *out, hipStream_t s) {
    return V == 1 ? launch_long<KIND, 1>(V, N, in, coef, st, out, s) : launch_long<KIND, 4>(V, N, in, coef, st, out, s);
}

int scan_long_check(const char *fn, int kind, size_t V, size_t N, const double *in, const double *coef, const double *st, const double *out) {
    if (kind < 0 || kind >= kLongKinds) return fail(MXG_ERR_INVALID, "%s: kind %d is none of 0 dc, 1 svf, 2 biquad, 3 lores, 4 hires, 5 lag", fn, kind);
    if (V < 1 || V > kLongMaxV) return fail(MXG_ERR_INVALID, "%s: V = %zu is outside 1 ... %zu", fn, V, kLongMaxV);
    if (N < 1 || N > kLongMaxN) return fail(MXG_ERR_INVALID, "%s: N = %zu is outside 1 ... 2^28", fn, N);
    if (!in || !coef || !st || !out) return fail(MXG_ERR_INVALID, "%s: a null pointer (in, coef, st, out)", fn);
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, bytes = N * V * sizeof(double);
    if (a != b && a < b + bytes && b < a + bytes)
        return fail(MXG_ERR_INVALID, "%s: out overlaps in partially (in place means out == in)", fn);
    return MXG_OK;
}

}  // namespace

int scan_long_host_render(int kind, size_t V, size_t N, const double *in, const double *coef, double *st, double *out);  // scan_long_host.cpp

}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_scan_long_render(int kind, size_t V, size_t N, const double *d_in, const double *d_coef, double *d_st, double *d_out, void *stream) {
    if (int s = scan_long_check(__func__, kind, V, N, d_in, d_coef, d_st, d_out)) return s;
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    hipStream_t st = resolve_stream(stream);
    switch (kind) {
        case 0: return launch_long_g<0>(V, N, d_in, d_coef, d_st, d_out, st);
        case 1: return launch_long_g<1>(V, N, d_in, d_coef, d_st, d_out, st);
        case 2: return launch_long_g<2>(V, N, d_in, d_coef, d_st, d_out, st);
        case 3: return launch_long_g<3>(V, N, d_in, d_coef, d_st, d_out, st);
        case 4: return launch_long_g<4>(V, N, d_in, d_coef, d_st, d_out, st);
        default: return launch_long_g<5>(V, N, d_in, d_coef, d_st, d_out, st);
    }
}

int mxg_scan_long_host(int kind, size_t V, size_t N, const double *h_in, const double *h_coef, double *h_st, double *h_out) {
    if (int s = scan_long_check(__func__, kind, V, N, h_in, h_coef, h_st, h_out)) return s;
    if (scan_long_host_render(kind, V, N, h_in, h_coef, h_st, h_out)) return fail(MXG_ERR_INVALID, "%s: out of host memory for the chunk states", __func__);
    return MXG_OK;
}

}  // extern "C"
