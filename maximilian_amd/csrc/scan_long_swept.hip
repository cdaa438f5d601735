// scan_long_swept.hip -- K31: K28's long time-parallel scan with PER-SAMPLE coefficients (mxg_scan_long_render_swept): a lores / hires
// whose cutoff and resonance move every sample, a maxiLagExp whose alpha does, over LONG signals of FEW voices.
//
// Path: maxiFilter::lores / hires C:455-484 and maxiLagExp<double>::addSample H:523-556 with the coefficients of every sample given
// by the caller, [N][rows][V], rows 0-1 read (what mxg_filter_render_coefs takes, rows = 3, or a packed rows = 2).  A voice's signal
// is cut into chunks of Ts = 1024 samples; every lane and every chunk carries an affine pair (M, e) of its own and the pairs are
// composed by scans, in three launches on the caller's stream (the arithmetic, the decomposition of N, the association order and
// the host twin whose bits these kernels must give: mxg_scan_long_swept.h):
//   A. scan_long_swept_summary_kernel  one wavefront per (chunk, voice), chunks 0 .. C-2: the chunk's pair, 6 doubles to scratch;
//   B. scan_long_swept_chunks_kernel   one wavefront per voice: the scan over the chunks' pairs, the true state after every chunk;
//   C. scan_long_swept_render_kernel   one wavefront per (chunk, voice): the block from the chunk's start state, the outputs; the last
//                                      chunk's wavefront renders the remainder (< 1024 samples) and stores the carried state.
// No workgroup waits on another: the order between the phases is stream order between launches; no flags, no atomics.  Scratch
// (SCR_SCAN_LONG_SWEPT, per stream, grow-only): pairs [V][C-1][6], states [V][C-1][2] -- voice-major, so that the lane of phase B that
// walks a run of consecutive chunks walks consecutive memory -- and [V][2] for the carried-in state, which phase A copies so that in
// phase C no workgroup reads the state array another one writes.
//
// Memory.  Lane k reads sample k L + i and its two coefficients: neighbouring lanes are L rows V doubles apart.  So phases A and C
// stage the chunk through LDS as K28 does, the input AND the two coefficient rows: the workgroup reads its tile with consecutive
// threads on consecutive addresses (inputs: runs of G doubles per row of [N][V]; coefficients: thread f takes voice f % G, row
// (f / G) % 2, sample f / 2G -- for V = 1 and rows = 2 one contiguous stream), writes three images per voice with the segment stride
// padded from 16 to 17 doubles, and lane k reads at 17 k + i: ds_read_b64, the 32 lanes of a half on 32 distinct 8-byte banks.  The
// images are 1096 doubles apart and the voices 3312 (8 and 16 mod 32), so that the staging writes of one instruction -- runs of
// consecutive doubles in up to four images -- fall on distinct banks as well.  The lane's passes (the pair, then the render) read x
// and the coefficients from the LDS image each time, so nothing of a segment lives in registers across the scan; phase C writes
// its outputs over the lane's own input segment and the workgroup stores the tile as it loaded it, so out == in works: a workgroup
// reads and writes its own tile only, and phase A has finished before phase C starts.  Algorithmic traffic per voice-sample:
// 8 (1 + rows) B read in A, the same in C, 8 B written (rows 0-1 are read; a third row shares their lines when V is small).
//
// Workgroups.  One voice's chunk is 3 x 1096 x 8 = 26 304 B of LDS, which is why Ts is 1024 and not K28's 2048: G = 1 wavefront
// (V = 1) gives 6 workgroups per CU in 160 KiB; G = 2 wavefronts (V >= 2), 52 800 B, gives 3 workgroups = 6 wavefronts per CU.
// K28's G = 4 would be 103 KiB: one workgroup per CU with nothing to overlap its barrier.
#include "mxg_common.h"
#include "mxg_scan_long_swept.h"

namespace mxg {
namespace {

constexpr int kSwSeg = kSweptL + 1;                   // a lane's 16 samples, padded: lane k at 17 k
constexpr int kSwImage = kScanLanes * kSwSeg + 8;     // one row's image: 1096 doubles, 8 mod 32
constexpr int kSwVoice = 3 * kSwImage + 24;           // a voice's three images (x, row 0, row 1): 3312 doubles, 16 mod 32
constexpr size_t kSweptMaxV = 4096, kSweptMaxN = (size_t)1 << 28;

__device__ __forceinline__ double sw_bcast(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
struct SweptWaveXch {  // the lane-exchange primitive of mxg_scan.h on a wavefront: one lane per executor (W = 1)
    int id;
    __device__ __forceinline__ int lane(int) const { return id; }
    __device__ __forceinline__ void up(const double (&src)[1], int d, double (&dst)[1]) const { dst[0] = __shfl_up(src[0], d); }
    __device__ __forceinline__ double from(const double (&src)[1], int j) const { return sw_bcast(src[0], j); }
};

__device__ __forceinline__ int sw_at(int t) { return t + (t >> 4); }  // sample t of a chunk in an image

// the workgroup's tile, samples [t0, t0 + 1024) x voices [v0, v0 + G): in from [N][V], rows 0-1 of coef from [N][rows][V]
template <int G>
__device__ __forceinline__ void sw_tile_load(double *tile, const double *in, const double *coef, size_t rows, size_t V, size_t v0, int tid) {
#pragma unroll 4
    for (int f = tid; f < kSweptChunk * G; f += kScanLanes * G) {
        const int t = f / G, g = f % G;
        if (v0 + g < V) tile[g * kSwVoice + sw_at(t)] = in[(size_t)t * V + v0 + g];
    }
#pragma unroll 4
    for (int f = tid; f < kSweptChunk * 2 * G; f += kScanLanes * G) {
        const int t = f / (2 * G), r = (f / G) % 2, g = f % G;
        if (v0 + g < V) tile[g * kSwVoice + (1 + r) * kSwImage + sw_at(t)] = coef[((size_t)t * rows + r) * V + v0 + g];
    }
}
template <int G>
__device__ __forceinline__ void sw_tile_store(const double *tile, double *out, size_t V, size_t v0, int tid) {
#pragma unroll 4
    for (int f = tid; f < kSweptChunk * G; f += kScanLanes * G) {
        const int t = f / G, g = f % G;
        if (v0 + g < V) out[(size_t)t * V + v0 + g] = tile[g * kSwVoice + sw_at(t)];
    }
}

template <int KIND>
__device__ __forceinline__ S3 sw_load_state(const double *st, size_t V, size_t v) {
    return S3{st[v], swept_dim(KIND) == 2 ? st[V + v] : 0.0, 0.0};
}

// A: grid (K, ceil(V / G)), chunk c = blockIdx.x < K = C - 1; pairs [V][K][6]; start0 [V][2]: the carried-in state, copied by chunk
// 0's wavefront for phase C
template <int KIND, int G>
__global__ __launch_bounds__(64 * G) void scan_long_swept_summary_kernel(size_t V, size_t K, size_t rows, const double *__restrict__ in,
                                                                          const double *__restrict__ coef, const double *__restrict__ st,
                                                                          double *__restrict__ pairs, double *__restrict__ start0) {
    extern __shared__ double tile[];
    const size_t c = blockIdx.x, v0 = (size_t)blockIdx.y * G;
    const int tid = threadIdx.x, g = tid / kScanLanes, lane = tid % kScanLanes;
    sw_tile_load<G>(tile, in + c * kSweptChunk * V, coef + c * kSweptChunk * rows * V, rows, V, v0, tid);
    __syncthreads();
    const size_t v = v0 + g;
    if (v >= V) return;
    const S3 s0 = c == 0 ? sw_load_state<KIND>(st, V, v) : S3{0.0, 0.0, 0.0};
    const double *img = tile + g * kSwVoice;
    const SweptPair p = swept_summary<KIND, kSweptL, 1>(SweptWaveXch{lane}, s0, [&](int, size_t n) { return img[sw_at((int)n)]; },
                                                        [&](int, size_t n, int r) { return img[(1 + r) * kSwImage + sw_at((int)n)]; });
    if (lane == 0) {
        double *o = pairs + (v * K + c) * kSweptPairDoubles;
        o[0] = p.M.m[0][0], o[1] = p.M.m[0][1], o[2] = p.M.m[1][0], o[3] = p.M.m[1][1], o[4] = p.e.a, o[5] = p.e.b;
        if (c == 0) start0[2 * v] = s0.a, start0[2 * v + 1] = s0.b;
    }
}

// B: grid V, one wavefront per voice; pairs [V][K][6] -> ends [V][K][2]
template <int KIND>
__global__ __launch_bounds__(64) void scan_long_swept_chunks_kernel(size_t K, const double *__restrict__ pairs, double *__restrict__ ends) {
    const size_t v = blockIdx.x;
    const double *P = pairs + v * K * kSweptPairDoubles;
    double *E = ends + v * K * kSweptEndDoubles;
    swept_chunks<swept_dim(KIND), 1>(SweptWaveXch{(int)threadIdx.x}, K,
                                     [&](size_t c) {
                                         const double *o = P + c * kSweptPairDoubles;
                                         SweptPair p = {};
                                         p.M.m[0][0] = o[0], p.M.m[0][1] = o[1], p.M.m[1][0] = o[2], p.M.m[1][1] = o[3], p.e.a = o[4], p.e.b = o[5];
                                         return p;
                                     },
                                     [&](size_t c, const S3 &q) { E[c * kSweptEndDoubles] = q.a, E[c * kSweptEndDoubles + 1] = q.b; });
}

// C: grid (max(C, 1), ceil(V / G)); ends [V][K][2] and start0 [V][2], K = C - 1 (unused when C <= 1); R = N % 1024.  st is read only
// when C <= 1, by the one workgroup of the voice that also writes it
template <int KIND, int G>
__global__ __launch_bounds__(64 * G) void scan_long_swept_render_kernel(size_t V, size_t C, size_t R, size_t rows, const double *in,
                                                                         const double *__restrict__ coef, double *__restrict__ st,
                                                                         const double *__restrict__ ends, const double *__restrict__ start0,
                                                                         double *out) {
    extern __shared__ double tile[];
    constexpr int D = swept_dim(KIND);
    const size_t c = blockIdx.x, v0 = (size_t)blockIdx.y * G;
    const int tid = threadIdx.x, g = tid / kScanLanes, lane = tid % kScanLanes;
    const size_t v = v0 + g;
    const bool live = v < V, chunk = c < C, last = c + 1 >= C;  // (chunk and last are the same in the whole workgroup)
    const SweptWaveXch xch{lane};
    S3 s = {0.0, 0.0, 0.0};
    if (live) {
        if (c == 0) s = C >= 2 ? S3{start0[2 * v], D == 2 ? start0[2 * v + 1] : 0.0, 0.0} : sw_load_state<KIND>(st, V, v);
        else {
            const double *E = ends + (v * (C - 1) + (c - 1)) * kSweptEndDoubles;
            s = S3{E[0], D == 2 ? E[1] : 0.0, 0.0};
        }
    }
    if (chunk) {
        sw_tile_load<G>(tile, in + c * kSweptChunk * V, coef + c * kSweptChunk * rows * V, rows, V, v0, tid);
        __syncthreads();
        if (live) {
            double *img = tile + g * kSwVoice;
            s = swept_block<KIND, kSweptL, 1>(xch, s, [&](int, size_t n) { return img[sw_at((int)n)]; },
                                              [&](int, size_t n, int r) { return img[(1 + r) * kSwImage + sw_at((int)n)]; },
                                              [&](int, size_t n, double y) { img[sw_at((int)n)] = y; });
        }
        __syncthreads();
        sw_tile_store<G>(tile, out + c * kSweptChunk * V, V, v0, tid);
    }
    if (!live || !last) return;
    const size_t n0 = C * kSweptChunk;  // the remainder: straight from global memory; a lane reads sample n before it writes output n
    const double *ip = in + n0 * V + v, *cp = coef + n0 * rows * V + v;
    double *op = out + n0 * V + v;
    s = swept_tail<KIND, 1>(xch, s, R, [&](int, size_t n) { return ip[n * V]; }, [&](int, size_t n, int r) { return cp[(n * rows + r) * V]; },
                            [&](int, size_t n, double y) { op[n * V] = y; }, [&](size_t n) { return ip[n * V]; },
                            [&](size_t n, int r) { return cp[(n * rows + r) * V]; }, [&](size_t n, double y) { if (lane == 0) op[n * V] = y; });
    if (lane == 0) {
        st[v] = s.a;
        if (D == 2) st[V + v] = s.b;
    }
}

template <int KIND, int G>
int launch_swept(size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out, hipStream_t s) {
    const size_t C = N / kSweptChunk, K = C > 1 ? C - 1 : 0, R = N % kSweptChunk;
    const size_t groups = (V + G - 1) / G;
    constexpr size_t lds = ((size_t)(G - 1) * kSwVoice + 3 * kSwImage) * sizeof(double);
    static_assert(lds <= 64 * 1024, "above 64 KiB of LDS a kernel has to be told");
    double *pairs = nullptr, *ends = nullptr, *start0 = nullptr;
    if (K) {
        void *p = nullptr;
        if (int rc = scratch_get(SCR_SCAN_LONG_SWEPT, s, ((kSweptPairDoubles + kSweptEndDoubles) * K + 2) * V * sizeof(double), &p)) return rc;
        pairs = (double *)p;
        ends = pairs + K * V * kSweptPairDoubles;
        start0 = ends + K * V * kSweptEndDoubles;
        {
            KernelTimer kt("scan_long_swept_summary_kernel", s);
            hipLaunchKernelGGL((scan_long_swept_summary_kernel<KIND, G>), dim3((unsigned)K, (unsigned)groups), dim3(64 * G), lds, s, V, K, rows, in, coef, st, pairs, start0);
        }
        MXG_HIP(hipGetLastError());
        {
            KernelTimer kt("scan_long_swept_chunks_kernel", s);
            hipLaunchKernelGGL((scan_long_swept_chunks_kernel<KIND>), dim3((unsigned)V), dim3(64), 0, s, K, pairs, ends);
        }
        MXG_HIP(hipGetLastError());
    }
    {
        KernelTimer kt("scan_long_swept_render_kernel", s);
        hipLaunchKernelGGL((scan_long_swept_render_kernel<KIND, G>), dim3((unsigned)(C ? C : 1), (unsigned)groups), dim3(64 * G), lds, s, V, C, R, rows, in, coef, st, ends, start0, out);
    }
    return check_hip(hipGetLastError(), "scan_long_swept_render_kernel launch");
}

template <int KIND>
int launch_swept_g(size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out, hipStream_t s) {
    return V == 1 ? launch_swept<KIND, 1>(V, N, in, coef, rows, st, out, s) : launch_swept<KIND, 2>(V, N, in, coef, rows, st, out, s);
}

int scan_long_swept_check(const char *fn, int kind, size_t V, size_t N, const double *in, const double *coef, size_t rows, const double *st, const double *out) {
    if (kind >= 0 && kind <= 2)
        return fail(MXG_ERR_INVALID, "%s: kind %d (0 dc, 1 svf, 2 biquad) has no swept form: no sequential per-sample entry point to alternate with; 3 lores, 4 hires and 5 lag have", fn, kind);
    if (!swept_kind(kind)) return fail(MXG_ERR_INVALID, "%s: kind %d is none of 3 lores, 4 hires, 5 lag", fn, kind);
    if (V < 1 || V > kSweptMaxV) return fail(MXG_ERR_INVALID, "%s: V = %zu is outside 1 ... %zu", fn, V, kSweptMaxV);
    if (N < 1 || N > kSweptMaxN) return fail(MXG_ERR_INVALID, "%s: N = %zu is outside 1 ... 2^28", fn, N);
    if (rows < (size_t)kSweptMinRows || rows > (size_t)kSweptMaxRows) return fail(MXG_ERR_INVALID, "%s: coef_rows = %zu is outside 2 ... 8", fn, rows);
    if (!in || !coef || !st || !out) return fail(MXG_ERR_INVALID, "%s: a null pointer (in, coef_ps, st, out)", fn);
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, k = (uintptr_t)coef, bytes = N * V * sizeof(double), kbytes = bytes * rows;
    if (a != b && a < b + bytes && b < a + bytes)
        return fail(MXG_ERR_INVALID, "%s: out overlaps in partially (in place means out == in)", fn);
    if (k < b + bytes && b < k + kbytes) return fail(MXG_ERR_INVALID, "%s: out overlaps coef_ps", fn);
    return MXG_OK;
}

}  // namespace

int scan_long_swept_host_render(int kind, size_t V, size_t N, const double *in, const double *coef, size_t rows, double *st, double *out);  // scan_long_swept_host.cpp

}  // namespace mxg

using namespace mxg;

extern "C" {

int mxg_scan_long_render_swept(int kind, size_t V, size_t N, const double *d_in, const double *d_coef_ps, size_t coef_rows, double *d_st,
                               double *d_out, void *stream) {
    if (int s = scan_long_swept_check(__func__, kind, V, N, d_in, d_coef_ps, coef_rows, d_st, d_out)) return s;
    if (int s = ensure_init()) return s;  // (after the argument checks: a refused call says why on a machine without a device too)
    hipStream_t st = resolve_stream(stream);
    switch (kind) {
        case 3: return launch_swept_g<3>(V, N, d_in, d_coef_ps, coef_rows, d_st, d_out, st);
        case 4: return launch_swept_g<4>(V, N, d_in, d_coef_ps, coef_rows, d_st, d_out, st);
        default: return launch_swept_g<5>(V, N, d_in, d_coef_ps, coef_rows, d_st, d_out, st);
    }
}

int mxg_scan_long_swept_host(int kind, size_t V, size_t N, const double *h_in, const double *h_coef_ps, size_t coef_rows, double *h_st,
                             double *h_out) {
    if (int s = scan_long_swept_check(__func__, kind, V, N, h_in, h_coef_ps, coef_rows, h_st, h_out)) return s;
    if (scan_long_swept_host_render(kind, V, N, h_in, h_coef_ps, coef_rows, h_st, h_out)) return fail(MXG_ERR_INVALID, "%s: out of host memory for the chunk pairs", __func__);
    return MXG_OK;
}

}  // extern "C"
